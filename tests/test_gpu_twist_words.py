"""`qg_twist_pack_words` / `qg_vec_observe_twisted_words`: the symmetry view of a packed observation written as packed 64-bit row words (a
packed -> packed bit gather through `obs_perms`), against a numpy reference written from the definition in include/qgym.h -- gather on the
dense bits, then pack -- which is itself cross-checked against `twist_expand_packed(..., int8)` packed on the host.  The shapes are the
smallest at which the mapping can go wrong: one env, a tail workgroup, several workgroups, a full 64-bit ballot, more than 64 words per env
(the lane-kept flush), byte words with an odd row count and a pad word, a single column, the 2 KiB LDS limit.  Then the exact pin through
the next kernel (`embed_words`, integer weights), the argument errors, and the handle path, eager and from a captured graph."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_embed_words import _int_weights  # noqa: E402
from test_gpu_vec_twists import make_vec, scrambled, twist_indices  # noqa: E402

WORD = {1: np.uint8, 4: np.uint32, 8: np.uint64}
TORCH_WORD = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
K = 3  # twists of the synthetic tables

SHAPES = [  # word_bytes, rows, cols, rows_out, batch
    (4, 6, 6, 6, 1),        # clifford 3q: a single-env workgroup
    (4, 6, 6, 6, 3),        # a few envs in one workgroup
    (4, 6, 6, 6, 67),       # a tail workgroup
    (4, 6, 6, 6, 300),      # several workgroups
    (8, 4, 64, 4, 5),       # a full ballot: bit 63
    (8, 70, 33, 70, 9),     # more than 64 words per env, not a multiple of 64: the lane-kept flush; cols crossing 32
    (1, 9, 9, 10, 20),      # byte words, odd rows: the pad word is written as 0, bits >= cols are 0
    (4, 8, 1, 8, 4),        # a single-column word
    (8, 256, 64, 256, 2),   # the 2 KiB LDS limit
]
IDS = [f"w{s[0]}-{s[1]}x{s[2]}-out{s[3]}-b{s[4]}" for s in SHAPES]


def random_words(rng, word_bytes, B, rows, cols):
    """Arbitrary words: every bit of a 4- / 8-byte word (those past `cols` must not show), bytes up to and past `cols` (they set nothing)."""
    if word_bytes == 1:
        return rng.integers(0, cols + 2, size=(B, rows)).astype(np.uint8)
    return rng.integers(0, 2**64, size=(B, rows), dtype=np.uint64).astype(WORD[word_bytes])


def dense_bits(words, cols):
    """What qg_expand_packed writes, [B, rows * cols] of {0, 1}: bit c of a word, or for byte words whether the byte is c."""
    c = np.arange(cols, dtype=np.uint64)
    if words.dtype == np.uint8:
        bits = words[:, :, None].astype(np.uint64) == c
    else:
        bits = (words[:, :, None].astype(np.uint64) >> c) & np.uint64(1)
    return bits.astype(np.uint8).reshape(words.shape[0], -1)


def gather(dense, table, t):
    """The definition of the view: entry i of env e is dense[e][table[t[e]][i]], 0 where that lies outside the observation; the env's own
    observation where t[e] is no twist."""
    obs = dense.shape[1]
    out = dense.copy()
    for e in range(dense.shape[0]):
        if 0 <= t[e] < len(table):
            src = table[t[e]].astype(np.int64)
            ok = (src >= 0) & (src < obs)
            out[e] = np.where(ok, dense[e][np.where(ok, src, 0)], 0)
    return out


def pack(dense, rows, cols, rows_out):
    """Dense [B, rows * cols] -> int64 [B, rows_out]: bit c of word r is entry r * cols + c, the words past `rows` are 0."""
    bits = dense.reshape(-1, rows, cols).astype(np.uint64)
    words = (bits << np.arange(cols, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    out = np.zeros((dense.shape[0], rows_out), dtype=np.uint64)
    out[:, :rows] = words
    return out.view(np.int64)


def reference(words, cols, table, t, rows_out):
    return pack(gather(dense_bits(words, cols), table, t), words.shape[1], cols, rows_out)


def on_device(words):
    return torch.as_tensor(words.view(np.int32) if words.dtype == np.uint32 else words.view(np.int64) if words.dtype == np.uint64 else words, device="cuda")


def run(words, cols, table, t, rows_out):
    """The kernel into a buffer of ones, and the cross-check of the reference: the dense view of the sibling kernel, packed here."""
    from qiskit_gym_amd.collector import twist_expand_packed, twist_pack_words

    B, rows = words.shape
    packed, tab, tw = on_device(words), torch.as_tensor(table, device="cuda"), torch.as_tensor(t, device="cuda")
    out = torch.full((B, rows_out), -1, dtype=torch.int64, device="cuda")
    got = twist_pack_words(packed, cols, tab, tw, rows_out=rows_out, out=out)
    assert got is out
    want = reference(words, cols, table, t, rows_out)
    sibling = twist_expand_packed(packed, cols, tab, tw, torch.int8)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(pack(sibling.cpu().numpy().astype(np.uint8), rows, cols, rows_out), want)
    return got.cpu().numpy(), want


@pytest.mark.parametrize("word_bytes,rows,cols,rows_out,B", SHAPES, ids=IDS)
def test_pack_words_is_the_packed_gather(word_bytes, rows, cols, rows_out, B):
    rng = np.random.default_rng(word_bytes * 100000 + rows * 100 + cols + B)
    words = random_words(rng, word_bytes, B, rows, cols)
    obs = rows * cols
    table = np.stack([rng.permutation(obs) for _ in range(K)]).astype(np.int32)
    indices = {
        "valid": rng.integers(0, K, size=B),
        "minus_one": np.full(B, -1),   # no such twist: the untwisted observation
        "n_twists": np.full(B, K),
        "mixed": rng.integers(-1, K + 1, size=B),
    }
    if B >= 4:
        indices["mixed"][:4] = [-1, K, 0, K - 1]
    for label, t in indices.items():
        got, want = run(words, cols, table, t.astype(np.int32), rows_out)
        np.testing.assert_array_equal(got, want, err_msg=label)
        if cols < 64:
            assert not (got.view(np.uint64) >> np.uint64(cols)).any(), label
        assert not got[:, rows:].any(), label
    if obs > 1:  # the view is not the observation
        assert (reference(words, cols, table, indices["valid"], rows_out) != reference(words, cols, table, indices["minus_one"], rows_out)).any()


def test_default_rows_out_is_the_even_row_count():
    from qiskit_gym_amd.collector import twist_pack_words

    rng = np.random.default_rng(2)
    for rows in (5, 6):
        words = random_words(rng, 4, 7, rows, 9)
        table = np.stack([rng.permutation(rows * 9) for _ in range(K)]).astype(np.int32)
        t = rng.integers(0, K, size=7).astype(np.int32)
        got = twist_pack_words(on_device(words), 9, torch.as_tensor(table, device="cuda"), torch.as_tensor(t, device="cuda"))
        assert got.dtype == torch.int64 and got.shape == (7, 6)
        np.testing.assert_array_equal(got.cpu().numpy(), reference(words, 9, table, t, 6))


@pytest.mark.parametrize("word_bytes,rows,cols,rows_out,B", [SHAPES[2], SHAPES[5], SHAPES[6]], ids=[IDS[2], IDS[5], IDS[6]])
def test_tables_that_are_not_permutations(word_bytes, rows, cols, rows_out, B):
    rng = np.random.default_rng(rows + cols)
    words = random_words(rng, word_bytes, B, rows, cols)
    obs = rows * cols
    table = np.zeros((K, obs), dtype=np.int32)
    table[0] = obs // 2  # every entry names the same source
    table[1] = rng.integers(0, obs, size=obs)  # sources repeat ...
    table[1][rng.random(obs) < 0.3] = -1       # ... and entries outside the observation read as 0
    table[1][rng.random(obs) < 0.3] = obs
    table[2] = rng.choice(np.array([-1, obs, obs + 7, 2**30, -2**31], dtype=np.int64), size=obs).astype(np.int32)  # nothing inside: all zero
    t = (np.arange(B) % K).astype(np.int32)
    got, want = run(words, cols, table, t, rows_out)
    np.testing.assert_array_equal(got, want)
    assert not got[t == 2].any()
    same = got[t == 0][:, :rows].view(np.uint64)
    full = np.uint64(2**cols - 1)
    assert ((same == 0) | (same == full)).all() and (same == same[:, :1]).all()  # one source bit, everywhere


@pytest.mark.parametrize("word_bytes,rows,cols,B", [(4, 6, 6, 67), (1, 9, 9, 300), (8, 70, 33, 9)])
def test_exact_through_the_first_layer(word_bytes, rows, cols, B):
    """`embed_words(twist_pack_words(...))` equals view_dense @ W.T + b exactly (weights +-1 and an integer bias: exact in bf16), for an even
    row count and for an odd one with the weight padded by `cols` zero columns."""
    from qiskit_gym_amd.collector import embed_words, pack_embed_words, twist_pack_words

    hidden = 128
    rng = np.random.default_rng(rows)
    words = random_words(rng, word_bytes, B, rows, cols)
    obs = rows * cols
    table = np.stack([rng.permutation(obs) for _ in range(K)]).astype(np.int32)
    t = rng.integers(-1, K + 1, size=B).astype(np.int32)
    view = torch.as_tensor(gather(dense_bits(words, cols), table, t).astype(np.float64), device="cuda")
    w, bias = _int_weights(hidden, obs, 5)
    wd, bd = w.cuda(), bias.cuda()
    rows_out = rows + rows % 2
    padded = torch.nn.functional.pad(wd, (0, cols)) if rows % 2 else wd
    got_words = twist_pack_words(on_device(words), cols, torch.as_tensor(table, device="cuda"), torch.as_tensor(t, device="cuda"))
    assert got_words.shape == (B, rows_out)
    out = embed_words(got_words, cols, pack_embed_words(padded, rows_out, cols), bd, hidden, relu=False)
    assert torch.equal(out.double(), view @ wd.double().t() + bd.double())


def test_pack_words_checks_its_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import twist_pack_words

    L = _lib.load()
    words = torch.zeros((4, 300), dtype=torch.int64, device="cuda")
    tab = torch.zeros((2, 64 * 64), dtype=torch.int32, device="cuda")
    tw = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 600), dtype=torch.int64, device="cuda")
    w, p, t, o = words.data_ptr(), tab.data_ptr(), tw.data_ptr(), out.data_ptr()
    call = L.qg_twist_pack_words
    assert call(w, 8, 4, 8, 8, p, 2, t, o, 8, None) == 0
    assert call(w, 8, 4, 8, 8, p, 2, t, o, 18, None) == 0  # 2 * rows + 2
    invalid = [(None, 8, 4, 8, 8, p, 2, t, o, 8), (w, 8, 4, 8, 8, None, 2, t, o, 8), (w, 8, 4, 8, 8, p, 2, None, o, 8), (w, 8, 4, 8, 8, p, 2, t, None, 8),
               (w, 8, 0, 8, 8, p, 2, t, o, 8), (w, 8, 4, 0, 8, p, 2, t, o, 8), (w, 8, 4, 8, 0, p, 2, t, o, 8), (w, 8, 4, 8, 8, p, 0, t, o, 8),
               (w, 2, 4, 8, 8, p, 2, t, o, 8),      # word_bytes
               (w, 8, 4, 8, 65, p, 2, t, o, 8),     # cols that do not fit the word
               (w, 4, 4, 8, 33, p, 2, t, o, 8),
               (w, 8, 4, 8, 8, p, 2, t, o + 4, 8),  # a misaligned output
               (w + 4, 8, 4, 8, 8, p, 2, t, o, 8)]
    for args in invalid:
        assert call(*args, None) == -1, args  # QG_ERR_INVALID
    unsupported = [(w, 1, 4, 8, 65, p, 2, t, o, 8),      # a byte names up to 256 columns, a 64-bit word of the view holds 64
                   (w, 8, 4, 8, 8, p, 2, t, o, 7),       # rows_out < rows
                   (w, 8, 4, 8, 8, p, 2, t, o, 19),      # rows_out > 2 * rows + 2
                   (w, 8, 4, 257, 1, p, 2, t, o, 257),   # more than 2 KiB of words per env
                   (w, 1, 4, 2048, 64, p, 16384, t, o, 2048)]  # a table of 2^31 entries
    for args in unsupported:
        assert call(*args, None) == -3, args  # QG_ERR_UNSUPPORTED
    small = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    tab8 = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
    assert twist_pack_words(small, 8, tab8, tw).shape == (4, 8)
    for bad in (lambda: twist_pack_words(small, 8, tab8, tw, rows_out=7),
                lambda: twist_pack_words(small, 8, tab8, tw, out=torch.zeros((4, 8), dtype=torch.int32, device="cuda")),
                lambda: twist_pack_words(small, 8, tab8, tw, out=torch.zeros((4, 10), dtype=torch.int64, device="cuda")),
                lambda: twist_pack_words(small, 8, tab8, tw[:3]),
                lambda: twist_pack_words(small, 8, tab8.long(), tw),
                lambda: twist_pack_words(small, 9, tab8, tw),                # the table is [n_twists, rows * cols]
                lambda: twist_pack_words(small.float(), 8, tab8, tw)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.QGymError) as e:
        twist_pack_words(small, 65, torch.zeros((2, 8 * 65), dtype=torch.int32, device="cuda"), tw)
    assert e.value.status == -1
    torch.cuda.synchronize()


def test_observe_twisted_words_needs_twists():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.envs.gateset import gateset_from_coupling_map
    from qiskit_gym_amd.vec import VecEnv
    from test_oracle_symmetry import GRAPHS
    from util import ALLOWED

    tw = torch.zeros(8, dtype=torch.int32, device="cuda")
    off = make_vec("lf_line5", batch=8, add_perms=False)
    with pytest.raises(_lib.QGymError) as e:
        off.observe_twisted_words(tw)
    assert e.value.status == -1
    n, edges = GRAPHS["ring6"]
    pauli = VecEnv("pauli", n, gateset_from_coupling_map(edges, None, ALLOWED["pauli"])[1], 8, add_perms=True, max_rotations=4, max_depth=32)
    with pytest.raises(_lib.QGymError) as e:
        pauli.observe_twisted_words(tw)
    assert e.value.status == -1
    on = make_vec("lf_line5", batch=8)
    for bad in (lambda: on.observe_twisted_words(tw[:4]), lambda: on.observe_twisted_words(tw.long()), lambda: on.observe_twisted_words(tw, rows_out=4),
                lambda: on.observe_twisted_words(tw, out=torch.zeros((8, 5), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    assert on.observe_twisted_words(tw).shape == (8, 6)


@pytest.mark.parametrize("case", ["clifford3_custom", "lf_line5", "perm_grid3x3"])
def test_the_handle_path_equals_observe_twisted_packed_on_the_host(case):
    """32-bit words with an even row count, a 5 x 5 observation, byte words with 9 rows: after a few random steps `observe_twisted_words` is
    `observe_twisted(int8)` packed; the same from a captured graph (after the eager call, which uploads the table) replayed on new states."""
    vec = make_vec(case)
    B, n_tw = vec.batch, vec.num_twists
    rows, cols = vec.obs_shape_
    rows_out = rows + rows % 2
    rng = scrambled(vec, 17)
    t = twist_indices(B, n_tw)
    tw = torch.as_tensor(t, device="cuda")

    def want():
        return pack(vec.observe_twisted(tw, torch.int8).cpu().numpy().astype(np.uint8), rows, cols, rows_out)

    got = vec.observe_twisted_words(tw)
    assert got.dtype == torch.int64 and got.shape == (B, rows_out)
    np.testing.assert_array_equal(got.cpu().numpy(), want())
    if n_tw > 1:
        assert (got.cpu().numpy() != pack(vec.observe().cpu().numpy().reshape(B, -1).astype(np.uint8), rows, cols, rows_out)).any()
    wide = torch.full((B, rows + 2), -1, dtype=torch.int64, device="cuda")  # any row count up to 2 * rows + 2: the rest is zero padding
    vec.observe_twisted_words(tw, rows_out=rows + 2, out=wide)
    np.testing.assert_array_equal(wide.cpu().numpy()[:, :rows_out], want())
    assert not wide[:, rows:].any()
    out = torch.full((B, rows_out), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vec.observe_twisted_words(tw, out=out)
    for r in range(2):
        vec.step(torch.as_tensor(rng.integers(0, vec.num_actions(), size=B), device="cuda", dtype=torch.int32))
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want(), err_msg=f"replay {r}")
    del graph
    vec.sync()
