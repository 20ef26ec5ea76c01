"""`collector.az_pack` (`qg_az_pack`) against the numpy restatement of tests/azmodel.py, bit for bit: random logs with monotone and
non-monotone live flags, rows of zeros, bad rows, rubbish in the columns of `counts` past A and in every output beforehand -- a sentinel shows
what the call does not write (ranks at or past n[0], the columns of pi past A).

The shapes cross every edge of the kernels' own geometry: 64 lanes, four actions per lane (64 / 65, 128 / 129, 192 / 193, 256 actions), the
chunk of 256 items a workgroup marks and writes (255 / 256 / 257 items), the 256 episodes a workgroup of the return scan takes (256 / 257),
the 256 chunks a pass of the chunk scan takes (65 536 / 65 537 items), the 64 words a pass of the word copy takes and the 2048-byte limit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from azmodel import pack  # noqa: E402
from test_azmodel import random_log  # noqa: E402
from test_gpu_mcts_kernels import bits  # noqa: E402

WORD = {1: (np.uint8, torch.uint8), 4: (np.int32, torch.int32), 8: (np.int64, torch.int64)}
SENTINEL = 0x7B  # every byte of every output before the call

# (T, E, A, W, word_bytes); W = 0: no words
SHAPES = [(1, 1, 1, 1, 8), (1, 1, 3, 0, 0), (3, 2, 8, 5, 1), (2, 63, 64, 2, 4), (2, 64, 65, 3, 4), (2, 65, 222, 1, 8), (5, 257, 170, 9, 1),
          (33, 130, 256, 6, 8),
          # four actions per lane: either side of every slice of 64
          (3, 5, 128, 0, 0), (3, 5, 129, 1, 1), (3, 5, 192, 0, 0), (3, 5, 193, 1, 4),
          # the chunk of 256 items, and the return scan's 256 episodes
          (1, 255, 3, 1, 1), (1, 256, 3, 1, 1), (1, 257, 3, 1, 1), (2, 256, 5, 0, 0),
          # the chunk scan's pass of 256 chunks
          (1, 65536, 3, 0, 0), (1, 65537, 3, 1, 1), (3, 21846, 2, 0, 0),
          # the word copy: 64 words a pass, and the most a sample may hold
          (3, 5, 8, 64, 1), (3, 5, 8, 65, 1), (2, 3, 4, 256, 8), (2, 3, 4, 2048, 1)]


def make_log(seed, T, E, A, W, wb, monotone):
    rng = np.random.default_rng(seed)
    counts, reward, live, move = random_log(rng, T, E, A, monotone=monotone, p_zero=0.1, p_bad=0.05)
    ld = A + 3
    wide = rng.integers(-9, 1 << 30, size=(T, E, ld)).astype(np.int32)  # rubbish, negative too, past A
    wide[:, :, :A] = counts
    words = None
    if W:
        words = rng.integers(0, 256, size=(T, E, W * wb), dtype=np.uint8).view(WORD[wb][0]).reshape(T, E, W)
    return wide, counts, reward, live, move, words


def sentinel_outputs(az, T, E, A, W, wb, cap, pi_ld):
    from qiskit_gym_amd import _lib

    u8 = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")  # noqa: E731
    pi = u8(cap * pi_ld * 4).view(torch.float32).view(cap, pi_ld)
    return az.AzPack(u8(12).view(torch.int32), u8(cap * 4).view(torch.int32), u8(cap * 4).view(torch.float32), u8(cap * 4).view(torch.int32),
                     pi[:, :A], u8(cap * W * wb).view(WORD[wb][1]).view(cap, W) if W else None,
                     u8(int(_lib.load().qg_az_pack_scratch_bytes(T, E)))), pi


def run_and_check(seed, T, E, A, W, wb, monotone, capacity=None, label=""):
    from qiskit_gym_amd import collector as az

    wide, counts, reward, live, move, words = make_log(seed, T, E, A, W, wb, monotone)
    cap = T * E if capacity is None else capacity
    dev = lambda x: None if x is None else torch.as_tensor(x, device="cuda")  # noqa: E731
    out, pi_full = sentinel_outputs(az, T, E, A, W, wb, cap, A + 2)
    res = az.az_pack(dev(wide)[:, :, :A], dev(reward), dev(live), dev(move), dev(words), capacity=capacity, out=out)
    torch.cuda.synchronize()
    want = pack(counts, reward, live, move, words, capacity=cap)
    n = res.n.cpu().numpy()
    np.testing.assert_array_equal(n, want.n, err_msg=f"{label}: n")
    k = int(n[0])
    np.testing.assert_array_equal(res.index.cpu().numpy()[:k], want.index, err_msg=f"{label}: index")
    np.testing.assert_array_equal(bits(res.z.cpu().numpy()[:k]), bits(want.z), err_msg=f"{label}: z")
    np.testing.assert_array_equal(res.move.cpu().numpy()[:k], want.move, err_msg=f"{label}: move")
    np.testing.assert_array_equal(bits(res.pi.cpu().numpy()[:k]), bits(want.pi), err_msg=f"{label}: pi")
    if W:
        np.testing.assert_array_equal(res.words.cpu().numpy()[:k], want.words, err_msg=f"{label}: words")
    # what is not written: every rank at or past n[0], and the columns of pi past A at every rank
    for name, t in (("index", res.index), ("z", res.z), ("move", res.move), ("words", res.words)):
        if t is not None:
            assert (t[k:].contiguous().view(torch.uint8) == SENTINEL).all(), f"{label}: {name} past n[0]"
    assert (pi_full[k:].contiguous().view(torch.uint8) == SENTINEL).all() and (pi_full[:, A:].contiguous().view(torch.uint8) == SENTINEL).all(), label
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(x) for x in s))
def test_against_the_model(shape):
    T, E, A, W, wb = shape
    seen = np.zeros(3, dtype=np.int64)
    for seed, monotone in ((0, True), (1, False)):
        want = run_and_check(seed + 10 * T + E, T, E, A, W, wb, monotone, label=f"{shape} monotone={monotone}")
        seen += want.n
    if T * E >= 64:  # the logs hold what the test is about: samples, and live rows that give none
        assert seen[0] > 0 and seen[2] > 0


def test_capacity_below_at_and_above_the_valid_decisions():
    T, E, A, W, wb = 5, 257, 7, 2, 4
    valid = int(run_and_check(3, T, E, A, W, wb, True).n[1])
    assert 300 < valid < T * E  # more than one chunk's worth, and dead rows among them
    for cap in (1, valid - 1, valid, valid + 1, T * E):
        want = run_and_check(3, T, E, A, W, wb, True, capacity=cap, label=f"capacity {cap}")
        assert want.n.tolist()[:2] == [min(cap, valid), valid]


def test_an_all_dead_log_and_a_log_of_one():
    from qiskit_gym_amd.collector import az_pack

    T, E, A = 4, 70, 5
    rng = np.random.default_rng(0)
    counts, reward, live, move = (torch.as_tensor(x, device="cuda") for x in random_log(rng, T, E, A, p_bad=0.3))
    res = az_pack(counts, reward, torch.zeros_like(live), move)
    assert res.n.tolist() == [0, 0, 0]
    res = az_pack(counts, reward, torch.zeros_like(live).bool(), move)  # bool flags are taken as they are
    assert res.n.tolist() == [0, 0, 0]
    one = az_pack(torch.tensor([[[2, 0, 6]]], dtype=torch.int32, device="cuda"), torch.tensor([[0.5]], device="cuda"),
                  torch.ones((1, 1), dtype=torch.uint8, device="cuda"), torch.tensor([[2]], dtype=torch.int32, device="cuda"))
    assert one.n.tolist() == [1, 1, 0] and one.pi.tolist() == [[0.25, 0.0, 0.75]] and one.z.tolist() == [0.5] and one.move.tolist() == [2]
    assert one.index.tolist() == [0] and one.words is None


def test_captured_into_a_graph_and_replayed_on_changed_inputs():
    from qiskit_gym_amd.collector import az_pack

    T, E, A, W = 6, 300, 37, 3
    logs = [make_log(s, T, E, A, W, 8, s % 2 == 0) for s in (1, 2, 3)]
    dev = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731
    ins = [dev(x) for x in (logs[0][0], logs[0][2], logs[0][3], logs[0][4], logs[0][5])]
    az_pack(ins[0][:, :, :A], *ins[1:])  # every kernel has run once before the capture
    torch.cuda.synchronize()
    graphed = az_pack(ins[0][:, :, :A], *ins[1:])  # the buffers the graph writes
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        az_pack(ins[0][:, :, :A], *ins[1:], out=graphed)
    for wide, counts, reward, live, move, words in logs[1:]:  # replayed twice, on other logs in the same buffers
        for t, x in zip(ins, (wide, reward, live, move, words)):
            t.copy_(dev(x))
        graph.replay()
        torch.cuda.synchronize()
        eager = az_pack(ins[0][:, :, :A], *ins[1:])
        torch.cuda.synchronize()
        want = pack(counts, reward, live, move, words)
        k = int(want.n[0])
        assert graphed.n.tolist() == eager.n.tolist() == want.n.tolist() and 0 < k < T * E
        for name in ("index", "z", "move", "pi", "words"):
            g, e = getattr(graphed, name)[:k], getattr(eager, name)[:k]
            assert g.contiguous().view(torch.uint8).equal(e.contiguous().view(torch.uint8)), name
        np.testing.assert_array_equal(bits(graphed.pi.cpu().numpy()[:k]), bits(want.pi))
        np.testing.assert_array_equal(bits(graphed.z.cpu().numpy()[:k]), bits(want.z))
        np.testing.assert_array_equal(graphed.index.cpu().numpy()[:k], want.index)


def test_every_error_as_its_code():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import az_pack

    L = _lib.load()
    T, E, A, W = 2, 3, 4, 2
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    buf = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    t = dict(counts=buf(T * E * A + 1, i32), reward=buf(T * E + 1, f32), live=buf(T * E, u8), move=buf(T * E + 1, i32), words=buf(T * E * W + 1, torch.int64),
             n=buf(4, i32), index=buf(T * E + 1, i32), z=buf(T * E + 1, f32), move_out=buf(T * E + 1, i32), pi=buf(T * E * A + 1, f32),
             words_out=buf(T * E * W + 1, torch.int64), scratch=buf(256, u8))
    good = dict(counts=t["counts"].data_ptr(), counts_ld=A, reward=t["reward"].data_ptr(), live=t["live"].data_ptr(), move=t["move"].data_ptr(),
                words=t["words"].data_ptr(), word_bytes=8, W=W, T=T, E=E, A=A, capacity=T * E, n=t["n"].data_ptr(), index=t["index"].data_ptr(),
                z=t["z"].data_ptr(), move_out=t["move_out"].data_ptr(), pi=t["pi"].data_ptr(), pi_ld=A, words_out=t["words_out"].data_ptr(),
                scratch=t["scratch"].data_ptr(), stream=None)

    def call(**kw):
        return L.qg_az_pack(*dict(good, **kw).values())

    assert call() == 0
    torch.cuda.synchronize()
    INVALID, UNSUPPORTED = -1, -3
    for name in ("counts", "reward", "live", "move", "n", "index", "z", "move_out", "pi", "scratch"):
        assert call(**{name: None}) == INVALID, name  # a null required pointer
    for name in ("T", "E", "A", "capacity"):
        assert call(**{name: 0}) == INVALID, name  # a zero size
    assert call(W=0) == INVALID
    assert call(counts_ld=A - 1) == INVALID and call(pi_ld=A - 1) == INVALID
    for wb in (0, 2, 3, 16, -1):
        assert call(word_bytes=wb) == INVALID, wb
    for name in ("counts", "reward", "move", "n", "index", "z", "move_out", "pi", "scratch"):
        assert call(**{name: good[name] + 2}) == INVALID, name  # a misaligned 32-bit array
    assert call(words=good["words"] + 4) == INVALID and call(words_out=good["words_out"] + 4) == INVALID  # the words: to word_bytes
    assert call(words_out=None) == INVALID  # words without words_out
    assert call(words=None, words_out=None, word_bytes=0, W=0) == 0  # no words at all is a call
    assert call(A=257, counts_ld=257, pi_ld=257) == UNSUPPORTED
    assert call(T=1 << 16, E=(1 << 15)) == UNSUPPORTED and call(T=2 ** 31 - 1, E=1) == UNSUPPORTED and call(T=1 << 40, E=1 << 40) == UNSUPPORTED
    assert call(W=257) == UNSUPPORTED and call(W=2049, word_bytes=1) == UNSUPPORTED and call(W=513, word_bytes=4) == UNSUPPORTED
    torch.cuda.synchronize()
    # the wrapper's own checks
    counts, reward, live, move = (torch.as_tensor(x, device="cuda") for x in random_log(np.random.default_rng(0), T, E, A))
    for bad in (dict(counts=counts.to(torch.int64)), dict(counts=counts[:, :, ::2]), dict(counts=counts.transpose(0, 1)), dict(reward=reward.double()),
                dict(reward=reward[:, :2]), dict(live=live.to(i32)), dict(move=move.to(torch.int64)), dict(move=move.t().contiguous().t()),
                dict(words=torch.zeros((T, E, 2), dtype=torch.int16, device="cuda")), dict(words=torch.zeros((T, E + 1, 2), dtype=u8, device="cuda")),
                dict(capacity=0), dict(reward=reward.cpu())):
        with pytest.raises(ValueError):
            az_pack(**dict(dict(counts=counts, reward=reward, live=live, move=move), **bad))
    first = az_pack(counts, reward, live, move)
    with pytest.raises(ValueError):
        az_pack(counts, reward, live, move, capacity=3, out=first)  # an `out` of another capacity
    with pytest.raises(_lib.QGymError) as e:
        az_pack(torch.zeros((1, 1, 257), dtype=i32, device="cuda"), buf(1, f32).view(1, 1), buf(1, u8).view(1, 1), buf(1, i32).view(1, 1))
    assert e.value.status == UNSUPPORTED
