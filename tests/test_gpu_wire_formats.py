"""`qg_vec_set_state` / `qg_vec_get_state` on every state layout at the calling patterns the rest of the suite never uses: strides wider
than the record, sources and destinations that are not 16-byte aligned, host destinations, and i64 entries at the values where `> 0 => 1`
(clifford.rs:299-304) can go wrong.  Batches 63 / 64 / 65 / 129 sit on both sides of the switch to the streaming kernels
(QG_STREAM_MIN_ENVS) and make `stride * B` odd and even.  Expected values come from tests/envmodel.py and tests/paulimodel.py; the records
are written and read by tests/wiremodel.py.  Every comparison is of integers or f32 bit patterns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import wiremodel as wm  # noqa: E402
from envmodel import Model  # noqa: E402
from paulimodel import PauliModel, to_wire  # noqa: E402
from test_dispatch import LAYOUT, OBS_DENSE, OBS_PACKED, STATE_I64, plan  # noqa: E402
from test_gpu_envmodel import _gateset  # noqa: E402
from test_paulimodel import random_labels, random_tableau  # noqa: E402
from util import f32_bits, line_gateset  # noqa: E402

PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
INVERTS = dict(add_inverts=True, add_perms=False, track_solution=False)
STREAMED = "row words / bit stream + streaming kernel"
DIRECT = "init / export kernel"
MAX_DEPTH = 128
BATCHES = (63, 64, 65, 129)
EXTRAS = (0, 1, 7)  # stride = the record + this many padding elements
FILLS = (-1, 1, 0x7F)
SENT = 0x5A  # every byte of a get_state destination before the call

LAYOUTS = [
    # kind, n, options, layout, dense / packed observation kernel at the natural stride (None: not a TILE configuration)
    ("clifford", 3, PLAIN, "TILE", "qm_dense_stream_any_kernel", "qm_pack_kernel"),
    ("clifford", 16, PLAIN, "TILE", "qm_dense_stream_kernel", "qm_pack_kernel"),
    ("linear_function", 9, PLAIN, "TILE", "qm_dense_stream_any_kernel", "qm_pack_kernel"),
    ("clifford", 17, PLAIN, "TILE64", None, None),
    ("linear_function", 33, PLAIN, "TILE64", None, None),
    ("linear_function", 64, PLAIN, "TILE64", None, None),
    ("linear_function", 9, INVERTS, "LFD", None, None),
    ("linear_function", 33, INVERTS, "LFD", None, None),
    ("linear_function", 5, PLAIN, "LF8", None, None),
    ("permutation", 9, PLAIN, "PERM", None, None),
    ("permutation", 17, PLAIN, "PERMB", None, None),
]
LAYOUT_IDS = [f"{c[3]}-{c[0]}{c[1]}" for c in LAYOUTS]


def _assert_routes(kind, n, opts, layout, dense_k, packed_k, B, A):
    assert plan(kind, n, LAYOUT, batch=B, num_actions=A, **opts) == layout
    streams = B >= 64 and layout in ("TILE", "TILE64", "LFD")
    assert plan(kind, n, STATE_I64, batch=B, num_actions=A, **opts) == (STREAMED if streams else DIRECT)
    if dense_k is not None:
        assert plan(kind, n, OBS_DENSE, batch=B, num_actions=A, **opts) == dense_k
        assert plan(kind, n, OBS_PACKED, batch=B, num_actions=A, **opts) == packed_k


def _make(kind, n, opts, B):
    from qiskit_gym_amd.vec import VecEnv

    gs = _gateset(kind, n)
    gv = VecEnv(kind, n, gs, B, max_depth=MAX_DEPTH, **opts)
    m = Model(kind, n, gs, B, add_inverts=opts["add_inverts"], track_solution=False, max_depth=MAX_DEPTH)
    return gs, gv, m


def _start(m, rng):
    """Each env's state: that of a random circuit; the identity in the first and the last env."""
    start = m.state_of_circuit(rng.integers(0, m.A, size=(m.B, 5)))
    start[0] = start[m.B - 1] = m.identity(1)[0]
    return start


def _draw(m, rng):
    acts = rng.integers(0, m.A, size=m.B)
    coins = rng.integers(0, 2, size=m.B) if m.add_inverts else np.zeros(m.B, np.int64)
    return acts, coins


def _step(gv, acts, coins):
    gv.step(torch.as_tensor(acts, device="cuda").to(torch.int32), torch.as_tensor(coins, device="cuda").to(torch.uint8) if gv.config["add_inverts"] else None)


def _snap(m):
    return dict(reward=f32_bits(m.reward).copy(), done=m.is_final().copy(), success=m.success.copy(), depth=m.depth.copy(),
                obs=m.observe().copy(), masks=m.masks().copy(), state=m.state.copy())


def _expect(gv, kind, n, snap, label, full=True):
    gv.sync()
    B = gv.batch
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), snap["reward"], err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), snap["done"], err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), snap["success"], err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), snap["depth"], err_msg=f"depth {label}")
    if not full:
        return
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(B, -1), snap["obs"], err_msg=f"observe {label}")
    words = wm.encode(kind, n, "packed", snap["state"], wm.min_elems(kind, n, "packed"))
    np.testing.assert_array_equal(gv.observe_packed().cpu().numpy().view(words.dtype), words, err_msg=f"observe_packed {label}")
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), snap["masks"], err_msg=f"masks {label}")


def _torch_view(a):
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])  # (torch has no unsigned words; the bits are what travels)


def _set_state(gv, rec, fmt, source):
    """qg_vec_set_state of the [B, stride] records `rec` from host memory ("host"), a fresh device tensor ("device": 16-byte aligned) or a
    contiguous device slice that starts one element into a larger allocation ("slice": aligned to the element, not to 16 bytes)."""
    from qiskit_gym_amd import _lib

    flat = _torch_view(np.ascontiguousarray(rec).reshape(-1))
    code, stride = wm.FORMAT_CODE[fmt], rec.shape[1]
    if source == "host":
        _lib.check(gv._L.qg_vec_set_state(gv._h, flat.ctypes.data, code, stride, 0, gv._stream()))
        return
    if source == "device":
        dev = torch.from_numpy(flat).cuda()
        assert dev.data_ptr() % 16 == 0
    else:
        big = torch.zeros(flat.size + 2, dtype=torch.from_numpy(flat[:1]).dtype, device="cuda")
        dev = big[1:1 + flat.size]
        dev.copy_(torch.from_numpy(flat))
        assert dev.is_contiguous() and dev.data_ptr() % 16 == flat.dtype.itemsize
    _lib.check(gv._L.qg_vec_set_state(gv._h, dev.data_ptr(), code, stride, 1, gv._stream()))
    torch.cuda.synchronize()  # (the source is read by the launches in flight)


def _sentinel(dtype):
    return int.from_bytes(bytes([SENT]) * dtype.itemsize, "little")


DESTINATIONS = ("device", "device_slice", "host", "host_slice")


def _get_state(gv, kind, n, fmt, stride, where):
    """qg_vec_get_state into a sentinel-filled buffer with guard space on both sides -> the [B, stride] records as they came back.
    "device": 16-byte aligned; "device_slice": one element past that; "host": 16-byte aligned; "host_slice": address 8 mod 16."""
    from qiskit_gym_amd import _lib

    dt = wm.elem_dtype(kind, n, fmt)
    nbytes = gv.batch * stride * dt.itemsize
    lead = {"device": 16, "device_slice": 16 + dt.itemsize, "host": 16, "host_slice": 24}[where]
    total = lead + nbytes + 32
    code = wm.FORMAT_CODE[fmt]
    if where.startswith("device"):
        big = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 16 == 0
        _lib.check(gv._L.qg_vec_get_state(gv._h, big.data_ptr() + lead, code, stride, 1, gv._stream()))
        torch.cuda.synchronize()
        raw = big.cpu().numpy()
    else:
        store = np.full(total + 16, SENT, np.uint8)
        off = (-store.ctypes.data) % 16
        raw = store[off:off + total]
        assert (raw.ctypes.data + lead) % 16 == (8 if where == "host_slice" else 0)
        _lib.check(gv._L.qg_vec_get_state(gv._h, raw.ctypes.data + lead, code, stride, 0, gv._stream()))
    assert (raw[:lead] == SENT).all(), f"written before the buffer ({fmt}, stride {stride}, {where})"
    assert (raw[lead + nbytes:] == SENT).all(), f"written past the buffer ({fmt}, stride {stride}, {where})"
    return raw[lead:lead + nbytes].copy().view(dt).reshape(gv.batch, stride)


def _records(kind, n, fmt, states, stride, fill, rng):
    rec = wm.encode(kind, n, fmt, states, stride, fill)
    if fmt == "i64" and kind != "permutation":
        rec = wm.spread_i64(rec, kind, n, rng)  # INT64_MIN, -1, 0 for a 0; 1, 2, 5, 1 << 32, 1 << 40, INT64_MAX for a 1
    return rec


# ---- set_state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind,n,opts,layout,dense_k,packed_k", LAYOUTS, ids=LAYOUT_IDS)
def test_set_state_formats_strides_and_sources(kind, n, opts, layout, dense_k, packed_k, B):
    gs, gv, m = _make(kind, n, opts, B)
    _assert_routes(kind, n, opts, layout, dense_k, packed_k, B, len(gs))
    rng = np.random.default_rng(1000 * n + B)
    start = _start(m, rng)
    # what the model says of the import and of two steps after it: the same for every way the records arrive
    m.set_state(m.wire(start))
    assert (m.depth == MAX_DEPTH).all() and m.success[0] and m.success[B - 1] and not m.success.all()
    snaps, steps = [_snap(m)], []
    for _ in range(2):
        steps.append(_draw(m, rng))
        m.step(*steps[-1])
        snaps.append(_snap(m))
    k = 0
    for fmt in wm.FORMATS:
        for extra in EXTRAS:
            for source in ("host", "device", "slice"):
                stride = wm.min_elems(kind, n, fmt) + extra
                fill = FILLS[k % 3]
                k += 1
                label = f"{fmt} stride min+{extra} fill {fill} from {source}"
                _set_state(gv, _records(kind, n, fmt, start, stride, fill, rng), fmt, source)
                _expect(gv, kind, n, snaps[0], f"import: {label}")
                for t, (acts, coins) in enumerate(steps):  # (LFD: the coins leave `inverted` set env by env for the next import to clear)
                    _step(gv, acts, coins)
                    _expect(gv, kind, n, snaps[t + 1], f"step {t}: {label}", full=t == 1)


# ---- get_state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind,n,opts,layout,dense_k,packed_k", LAYOUTS, ids=LAYOUT_IDS)
def test_get_state_formats_strides_and_destinations(kind, n, opts, layout, dense_k, packed_k, B):
    gs, gv, m = _make(kind, n, opts, B)
    _assert_routes(kind, n, opts, layout, dense_k, packed_k, B, len(gs))
    rng = np.random.default_rng(2000 * n + B)
    start = _start(m, rng)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    for _ in range(3):  # LFD: random coins, so that the side the export has to read differs env by env
        acts, coins = _draw(m, rng)
        m.step(acts, coins)
        _step(gv, acts, coins)
    if m.add_inverts:
        assert m.inverted.any() and not m.inverted.all()
    gv.sync()
    for fmt in wm.FORMATS:
        sentinel = _sentinel(wm.elem_dtype(kind, n, fmt))
        for extra in EXTRAS:
            stride = wm.min_elems(kind, n, fmt) + extra
            for where in DESTINATIONS:
                rec = _get_state(gv, kind, n, fmt, stride, where)
                got = wm.decode(kind, n, fmt, rec, stride, sentinel)  # (asserts that the padding is still the sentinel)
                np.testing.assert_array_equal(got, m.state, err_msg=f"{fmt} stride min+{extra} into {where}")


# ---- get_state -> set_state -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", wm.FORMATS)
@pytest.mark.parametrize("B", (63, 65))
@pytest.mark.parametrize("kind,n,opts,layout,dense_k,packed_k", LAYOUTS, ids=LAYOUT_IDS)
def test_round_trip_through_a_padded_buffer(kind, n, opts, layout, dense_k, packed_k, B, fmt):
    from qiskit_gym_amd import _lib

    gs, ga, m = _make(kind, n, opts, B)
    _, gb, _ = _make(kind, n, opts, B)
    rng = np.random.default_rng(3000 * n + B)
    start = _start(m, rng)
    ga.set_state(m.wire(start))
    for _ in range(3):  # LFD: the export must follow each env's `inverted` flag, and the import into `gb` clears it
        _step(ga, *_draw(m, rng))
    dt = wm.elem_dtype(kind, n, fmt)
    stride = wm.min_elems(kind, n, fmt) + 7
    buf = torch.from_numpy(_torch_view(np.full(B * stride, _sentinel(dt), dtype=dt))).cuda()
    code = wm.FORMAT_CODE[fmt]
    _lib.check(ga._L.qg_vec_get_state(ga._h, buf.data_ptr(), code, stride, 1, ga._stream()))
    _lib.check(gb._L.qg_vec_set_state(gb._h, buf.data_ptr(), code, stride, 1, gb._stream()))
    torch.cuda.synchronize()
    wm.decode(kind, n, fmt, buf.cpu().numpy().view(dt), stride, _sentinel(dt))  # a well-formed record, padding untouched by either call
    for t in range(3):
        if t:
            acts, coins = _draw(m, rng)
            _step(ga, acts, coins)
            _step(gb, acts, coins)
        ga.sync()
        gb.sync()
        np.testing.assert_array_equal(ga.get_state("packed").cpu().numpy(), gb.get_state("packed").cpu().numpy(), err_msg=f"state t={t}")
        np.testing.assert_array_equal(ga.observe().cpu().numpy(), gb.observe().cpu().numpy(), err_msg=f"observe t={t}")
        np.testing.assert_array_equal(ga.success.cpu().numpy(), gb.success.cpu().numpy(), err_msg=f"success t={t}")
        if t:  # (`ga` is three steps into its episode, `gb` at the start of one: after the import only what a step computes is equal)
            np.testing.assert_array_equal(f32_bits(ga.reward.cpu().numpy()), f32_bits(gb.reward.cpu().numpy()), err_msg=f"reward t={t}")
            np.testing.assert_array_equal(ga.done.cpu().numpy(), gb.done.cpu().numpy(), err_msg=f"done t={t}")
    assert (gb.depth.cpu().numpy() == MAX_DEPTH - 2).all()


# ---- PauliEnv -------------------------------------------------------------------------------------------------------------
PAULI = dict(add_perms=False, track_solution=False, max_rotations=3, max_depth=MAX_DEPTH)


def _pauli_pair(B, n=4):
    from qiskit_gym_amd.vec import VecEnv

    gs = line_gateset("pauli", n)
    assert str(plan("pauli", n, LAYOUT, batch=B, num_actions=len(gs), **PAULI)).startswith("PTILE")
    assert plan("pauli", n, STATE_I64, batch=B, num_actions=len(gs), **PAULI) == (STREAMED if B >= 64 else DIRECT)
    gv = VecEnv("pauli", n, gs, B, **PAULI)
    m = PauliModel(n, gs, B, max_rotations=3, add_perms=False, track_solution=False, max_depth=MAX_DEPTH)
    return n, gs, gv, m


def _pauli_wires(n, B, rng, rotations=True):
    wires = []
    for b in range(B):
        tab = np.eye(2 * n, dtype=np.uint8) if b in (0, B - 1) else random_tableau(rng, n, int(rng.integers(1, 2 * n)))
        labels = random_labels(rng, n, int(rng.integers(0, 4)), 4) if rotations and b not in (0, B - 1) else []
        wires.append(to_wire(tab, labels))
    return wires


def _pauli_expect(gv, m, label):
    gv.sync()
    B = m.B
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), m.success, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth {label}")
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), m.masks(), err_msg=f"masks {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(B, -1), m.observe(), err_msg=f"observe {label}")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), m.tableau(), err_msg=f"tableau {label}")


@pytest.mark.parametrize("B", BATCHES)
def test_pauli_set_state_padded_and_get_state_everywhere(B):
    n, gs, gv, m = _pauli_pair(B)
    rng = np.random.default_rng(B)
    wires = _pauli_wires(n, B, rng)
    width = max(len(w) for w in wires)
    tab_end = 1 + 4 * n * n
    k = 0
    for extra in EXTRAS:
        for source in ("host", "device", "slice"):
            fill = FILLS[k % 3]
            k += 1
            rec = np.full((B, width + extra), fill, np.int64)  # (a record names its own length: what follows the last rotation is padding)
            for b, w in enumerate(wires):
                rec[b, : len(w)] = w
            ones = np.array(wm.I64_ONES, np.int64)[rng.integers(0, len(wm.I64_ONES), size=(B, tab_end - 1))]
            zeros = np.array(wm.I64_ZEROS, np.int64)[rng.integers(0, len(wm.I64_ZEROS), size=(B, tab_end - 1))]
            rec[:, 1:tab_end] = np.where(rec[:, 1:tab_end] > 0, ones, zeros)  # pauli.rs:527: `> 0`
            label = f"stride {width}+{extra} fill {fill} from {source}"
            _set_state(gv, rec, "i64", source)
            m.set_state(wires)
            _pauli_expect(gv, m, f"import: {label}")
            assert (m.depth == MAX_DEPTH).all() and m.success[0] and m.success[B - 1]
            for t in range(2):
                acts = rng.integers(0, len(gs), size=B)
                m.step(acts)
                gv.step(torch.as_tensor(acts, device="cuda").to(torch.int32))
                _pauli_expect(gv, m, f"step {t}: {label}")
    want = m.tableau().reshape(B, 2 * n, 2 * n).astype(np.uint8)
    for fmt in wm.FORMATS:
        sentinel = _sentinel(wm.elem_dtype("pauli", n, fmt))
        for extra in EXTRAS:
            stride = wm.min_elems("pauli", n, fmt) + extra
            for where in DESTINATIONS:
                rec = _get_state(gv, "pauli", n, fmt, stride, where)
                np.testing.assert_array_equal(wm.decode("pauli", n, fmt, rec, stride, sentinel), want, err_msg=f"{fmt} stride min+{extra} into {where}")


@pytest.mark.parametrize("n", (5, 6))
def test_pauli_get_state_of_rows_longer_than_their_word(n):
    """2n = 10 or 12 columns: a dense row has more bytes than the 8-byte word it is expanded from, so an expansion that shared its buffer
    with the row words (the staging buffer of a host destination) would read words it has already overwritten."""
    B = 65
    _, gs, gv, m = _pauli_pair(B, n)
    rng = np.random.default_rng(n)
    wires = _pauli_wires(n, B, rng)
    width = max(len(w) for w in wires)
    gv.set_state(np.array([w + [0] * (width - len(w)) for w in wires], np.int64))
    m.set_state(wires)
    want = m.tableau().reshape(B, 2 * n, 2 * n).astype(np.uint8)
    for fmt in wm.FORMATS:
        sentinel = _sentinel(wm.elem_dtype("pauli", n, fmt))
        for extra in (0, 1):
            stride = wm.min_elems("pauli", n, fmt) + extra
            for where in DESTINATIONS:
                rec = _get_state(gv, "pauli", n, fmt, stride, where)
                np.testing.assert_array_equal(wm.decode("pauli", n, fmt, rec, stride, sentinel), want, err_msg=f"{fmt} stride min+{extra} into {where}")


def test_pauli_get_state_into_host_memory_at_a_batch_of_many_workgroups():
    """The constructor state (identity tableaus) of 4 097 envs of 6 qubits, as u8 and i64 into host memory: 590 KB that the expansion
    kernel writes from 36 workgroups.  When it wrote them into the buffer that also held its row words, some 760 envs came back wrong
    at this size (none at 65 envs, where every wave had read its words before any other wrote)."""
    from qiskit_gym_amd.vec import VecEnv

    n, B = 6, 4097
    gv = VecEnv("pauli", n, line_gateset("pauli", n), B, **PAULI)
    want = np.broadcast_to(np.eye(2 * n, dtype=np.uint8), (B, 2 * n, 2 * n))
    for fmt in wm.FORMATS:
        sentinel = _sentinel(wm.elem_dtype("pauli", n, fmt))
        for where in ("host", "host_slice", "device"):
            stride = wm.min_elems("pauli", n, fmt)
            rec = _get_state(gv, "pauli", n, fmt, stride, where)
            got = wm.decode("pauli", n, fmt, rec, stride, sentinel)
            assert not (got != want).any(axis=(1, 2)).sum(), f"{fmt} into {where}: {(got != want).any(axis=(1, 2)).sum()} envs are not the identity"


@pytest.mark.parametrize("B", (63, 65))
def test_pauli_round_trip_of_the_tableau(B):
    """get_state returns the tableau alone, so the record set_state reads is built around it: the rotation count (0) in the element before
    each env's tableau, which get_state writes at a stride of 1 + 64 + 7."""
    from qiskit_gym_amd import _lib

    n, gs, ga, m = _pauli_pair(B)
    _, _, gb, _ = _pauli_pair(B)
    rng = np.random.default_rng(B)
    ga.set_state(np.array(_pauli_wires(n, B, rng, rotations=False), np.int64))
    for _ in range(3):
        ga.step(torch.as_tensor(rng.integers(0, len(gs), size=B), device="cuda").to(torch.int32))
    stride = 1 + wm.min_elems("pauli", n, "i64") + 7
    buf = torch.zeros(B * stride + 1, dtype=torch.int64, device="cuda")
    _lib.check(ga._L.qg_vec_get_state(ga._h, buf.data_ptr() + 8, 0, stride, 1, ga._stream()))
    _lib.check(gb._L.qg_vec_set_state(gb._h, buf.data_ptr(), 0, stride, 1, gb._stream()))
    torch.cuda.synchronize()
    for t in range(3):
        if t:
            acts = torch.as_tensor(rng.integers(0, len(gs), size=B), device="cuda").to(torch.int32)
            ga.step(acts)
            gb.step(acts)
        ga.sync()
        gb.sync()
        for fmt in wm.FORMATS:
            np.testing.assert_array_equal(ga.get_state(fmt).cpu().numpy(), gb.get_state(fmt).cpu().numpy(), err_msg=f"{fmt} t={t}")
        np.testing.assert_array_equal(ga.success.cpu().numpy(), gb.success.cpu().numpy(), err_msg=f"success t={t}")
        if t:
            np.testing.assert_array_equal(f32_bits(ga.reward.cpu().numpy()), f32_bits(gb.reward.cpu().numpy()), err_msg=f"reward t={t}")
            np.testing.assert_array_equal(ga.done.cpu().numpy(), gb.done.cpu().numpy(), err_msg=f"done t={t}")


# ---- refusals -------------------------------------------------------------------------------------------------------------
REFUSALS = [LAYOUTS[0], LAYOUTS[4], LAYOUTS[7], LAYOUTS[8], LAYOUTS[9], LAYOUTS[10]]


@pytest.mark.parametrize("kind,n,opts,layout,dense_k,packed_k", REFUSALS, ids=[f"{c[3]}-{c[0]}{c[1]}" for c in REFUSALS])
def test_refused_calls_leave_the_state_alone(kind, n, opts, layout, dense_k, packed_k):
    from qiskit_gym_amd import _lib

    B = 65
    gs, gv, m = _make(kind, n, opts, B)
    rng = np.random.default_rng(n)
    start = _start(m, rng)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    snap = _snap(m)
    other = wm.encode(kind, n, "i64", m.identity(B), wm.min_elems(kind, n, "i64"))
    big = torch.full((B * (wm.min_elems(kind, n, "i64") + 8),), _sentinel(np.dtype(np.int64)), dtype=torch.int64, device="cuda")
    src = torch.from_numpy(np.ascontiguousarray(other)).cuda()
    for fmt in wm.FORMATS:
        short = wm.min_elems(kind, n, fmt) - 1
        code = wm.FORMAT_CODE[fmt]
        for on_device, ptr in ((1, src.data_ptr()), (0, other.ctypes.data)):
            with pytest.raises(_lib.QGymError, match="elements per env"):
                _lib.check(gv._L.qg_vec_set_state(gv._h, ptr, code, short, on_device, gv._stream()))
        with pytest.raises(_lib.QGymError, match="stride"):
            _lib.check(gv._L.qg_vec_get_state(gv._h, big.data_ptr(), code, short, 1, gv._stream()))
    for code in (-1, 3, 7):
        with pytest.raises(_lib.QGymError, match="unknown state format"):
            _lib.check(gv._L.qg_vec_set_state(gv._h, src.data_ptr(), code, wm.min_elems(kind, n, "i64"), 1, gv._stream()))
        with pytest.raises(_lib.QGymError, match="unknown state format"):
            _lib.check(gv._L.qg_vec_get_state(gv._h, big.data_ptr(), code, wm.min_elems(kind, n, "i64"), 1, gv._stream()))
    torch.cuda.synchronize()
    assert (big == _sentinel(np.dtype(np.int64))).all()
    _expect(gv, kind, n, snap, "after the refusals")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), m.wire())


def test_pauli_refusals_leave_the_state_alone():
    from qiskit_gym_amd import _lib

    B = 65
    n, gs, gv, m = _pauli_pair(B)
    rng = np.random.default_rng(5)
    wires = _pauli_wires(n, B, rng)
    width = max(len(w) for w in wires)
    rec = np.array([w + [0] * (width - len(w)) for w in wires], np.int64)
    gv.set_state(rec)
    m.set_state(wires)
    src = torch.zeros(B * 64, dtype=torch.int64, device="cuda")
    big = torch.full((B * 72,), _sentinel(np.dtype(np.int64)), dtype=torch.int64, device="cuda")
    for fmt in ("u8", "packed"):
        for on_device, ptr in ((1, src.data_ptr()), (0, rec.ctypes.data)):
            with pytest.raises(_lib.QGymError, match="i64 wire format only"):
                _lib.check(gv._L.qg_vec_set_state(gv._h, ptr, wm.FORMAT_CODE[fmt], wm.min_elems("pauli", n, fmt), on_device, gv._stream()))
    for fmt in wm.FORMATS:
        with pytest.raises(_lib.QGymError, match="stride"):
            _lib.check(gv._L.qg_vec_get_state(gv._h, big.data_ptr(), wm.FORMAT_CODE[fmt], wm.min_elems("pauli", n, fmt) - 1, 1, gv._stream()))
    for code in (-1, 3):
        with pytest.raises(_lib.QGymError, match="unknown state format"):
            _lib.check(gv._L.qg_vec_set_state(gv._h, src.data_ptr(), code, 65, 1, gv._stream()))
        with pytest.raises(_lib.QGymError, match="unknown state format"):
            _lib.check(gv._L.qg_vec_get_state(gv._h, big.data_ptr(), code, 64, 1, gv._stream()))
    torch.cuda.synchronize()
    assert (big == _sentinel(np.dtype(np.int64))).all()
    _pauli_expect(gv, m, "after the refusals")
