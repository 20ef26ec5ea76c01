"""`BatchedSynthesis.self_play` beside `solve(mcts_sampled=True)` with the same arguments, in the same process, alternating, with the
reference's trained policies (tests/golden/policies): episodes and samples per second, and what logging and packing cost -- the difference of
the two times (a host clock around calls that end in a synchronise; every call made once untimed, then `--repeats` timed pairs, the median
kept and the spread printed).  Rows: the three golden policies x N in {8, 32} x K in {1, 4}; the targets are random scrambles made on the
device, read back once so that both calls get the same states.
Then `az_pack` alone, between device events, on the log of the last self-play of each row and on a synthetic log of a training-sized
collection (T = 32 decisions x 65 536 episodes, half the rows live), beside a tensor-library restatement of rules 1-5 (`torch_pack`: totals,
flags, a reverse cumulative sum for z, nonzero / index_select for the order, a division for pi) in the same process; both are checked against
each other before they are timed (z within f32 rounding of the different summation order, pi within one rounding of the library's division,
everything else exactly).
A record, not a gate.  Run on the GPU box: python tools/bench_self_play.py [--episodes 1024] [--difficulty 20] [--only NAME] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_reference_policies import MODELS, load  # noqa: E402

import qiskit_gym_amd.envs as envs  # noqa: E402
from qiskit_gym_amd.collector import az_pack  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}
NAMES = ("clifford_3q_custom", "lf_5_line", "perm_square_3x3")
SIMS, LEAVES = (8, 32), (1, 4)


def gym_of(name):
    cfg, gateset, w = load(name)
    gym = getattr(envs, GYMS[MODELS[name]])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    return gym, policy_from_reference_state_dict(w)


def drop_handles(syn):
    for held in list(syn._held):
        for vec in syn._held.pop(held).vecs:
            vec.close()


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def torch_pack(counts, reward, live, move, words):
    """Rules 1-5 of qg_az_pack on the tensor library (capacity = T * E).  z is a reverse cumulative sum: the same numbers in another
    summation order, so it agrees with the kernel within rounding, not bit for bit."""
    T, E, A = counts.shape
    alive = live != 0
    total = counts.to(torch.int64).sum(dim=2)
    bad = alive & ((counts < 0).any(dim=2) | (total >= 1 << 24))
    valid = alive & ~bad & (total > 0)
    g = torch.flip(torch.cumsum(torch.flip(torch.where(alive, reward, torch.zeros_like(reward)), (0,)), 0), (0,))
    index = torch.nonzero(valid.reshape(-1)).squeeze(1)
    pi = counts.reshape(T * E, A).index_select(0, index).to(torch.float32) / total.reshape(-1).index_select(0, index).to(torch.float32).unsqueeze(1)
    n = torch.stack([valid.sum(), valid.sum(), bad.sum()]).to(torch.int32)
    return (n, index.to(torch.int32), g.reshape(-1).index_select(0, index), move.reshape(-1).index_select(0, index), pi,
            None if words is None else words.reshape(T * E, -1).index_select(0, index))


def pack_row(label, counts, reward, live, move, words, repeats, out):
    T, E, A = counts.shape
    mine = az_pack(counts, reward, live, move, words)
    ref = torch_pack(counts, reward, live, move, words)
    k = int(mine.n[0])
    assert mine.n.tolist() == ref[0].tolist() and mine.index[:k].equal(ref[1]) and mine.move[:k].equal(ref[3])
    assert torch.allclose(mine.pi[:k], ref[4], rtol=1e-6, atol=0) and (words is None or mine.words[:k].equal(ref[5]))  # (the library's division may round otherwise)
    assert torch.allclose(mine.z[:k], ref[2], rtol=1e-4, atol=1e-4)
    kernel = event_ms(lambda: az_pack(counts, reward, live, move, words, out=mine), repeats)
    library = event_ms(lambda: torch_pack(counts, reward, live, move, words), repeats)
    live_rows = int((live != 0).sum())
    row = dict(what="az_pack", log=label, T=T, E=E, A=A, live_rows=live_rows, samples=k, kernel_ms=kernel[0], kernel_ms_range=kernel[1:], torch_ms=library[0],
               torch_ms_range=library[1:], counts_bytes=T * E * A * 4, live_counts_bytes=live_rows * A * 4)
    out.append(row)
    print(f"az_pack, {label}: T={T} E={E} A={A}, {live_rows} live rows, {k} samples: kernels {kernel[0]:.3f} ms ({kernel[1]:.3f} .. {kernel[2]:.3f}), "
          f"tensor library {library[0]:.3f} ms ({library[1]:.3f} .. {library[2]:.3f}); counts log {T * E * A * 4 / 1e6:.1f} MB, of live rows "
          f"{live_rows * A * 4 / 1e6:.1f} MB", flush=True)


def table(E: int, difficulty: int, names, repeats, out):
    for name in names:
        gym, policy = gym_of(name)
        syn = BatchedSynthesis(gym, policy, seed=1)
        v = gym.vec(E, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)
        states = v.get_state("i64").cpu().numpy()
        v.close()
        for N in SIMS:
            for K in LEAVES:
                kw = dict(num_mcts_searches=N)
                if K > 1:
                    kw.update(mcts_leaves=K)
                play = lambda: syn.self_play(states=states, **kw)  # noqa: E731
                solve = lambda: syn.solve(states, num_searches=1, mcts_sampled=True, **kw)  # noqa: E731
                batch = play()  # every code path and handle once, untimed
                solve()
                pairs = [(host_ms(play), host_ms(solve)) for _ in range(repeats)]  # alternating
                sp, so = statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)
                st = batch.stats
                row = dict(what="self_play", policy=name, episodes=E, difficulty=difficulty, N=N, K=K, self_play_ms=sp, solve_ms=so, logging_ms=sp - so,
                           self_play_ms_range=[min(p[0] for p in pairs), max(p[0] for p in pairs)], solve_ms_range=[min(p[1] for p in pairs), max(p[1] for p in pairs)],
                           decisions=st["steps"], samples=st["samples"], episodes_solved=st["episodes_solved"], episodes_per_s=E / sp * 1e3,
                           samples_per_s=st["samples"] / sp * 1e3)
                out.append(row)
                print(f"{name} x {E} (difficulty {difficulty}), N={N}, K={K}: self_play {sp:.1f} ms ({row['self_play_ms_range'][0]:.1f} .. "
                      f"{row['self_play_ms_range'][1]:.1f}), solve(mcts_sampled) {so:.1f} ms ({row['solve_ms_range'][0]:.1f} .. {row['solve_ms_range'][1]:.1f}), "
                      f"logging and packing {sp - so:+.1f} ms; {st['steps']} decisions, {st['samples']} samples, {st['episodes_solved']:.1%} solved; "
                      f"{row['episodes_per_s']:.0f} episodes/s, {row['samples_per_s']:.0f} samples/s", flush=True)
            log = syn._held["self-play-many"].log
            steps = batch.stats["steps"]
            pack_row(f"{name} N={N} K={LEAVES[-1]}", log.counts[:steps], log.reward[:steps], log.live[:steps].view(torch.uint8), log.move[:steps], log.words[:steps],
                     repeats, out)
            drop_handles(syn)


def synthetic(repeats, out, T=32, E=65536, A=40, W=5):
    g = torch.Generator(device="cuda").manual_seed(0)
    counts = torch.randint(0, 9, (T, E, A), generator=g, device="cuda", dtype=torch.int32)
    live = (torch.arange(T, device="cuda")[:, None] < torch.randint(0, T + 1, (E,), generator=g, device="cuda")[None, :]).to(torch.uint8)
    reward = torch.randn((T, E), generator=g, device="cuda")
    move = torch.randint(0, A, (T, E), generator=g, device="cuda", dtype=torch.int32)
    words = torch.randint(0, 1 << 40, (T, E, W), generator=g, device="cuda", dtype=torch.int64)
    pack_row("synthetic", counts, reward, live, move, words, repeats, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=NAMES, action="append", help="these policies alone")
    ap.add_argument("--json", help="the rows, as JSON, into this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rows = []
    try:
        table(args.episodes, args.difficulty, args.only or NAMES, args.repeats, rows)
        synthetic(max(args.repeats, 10), rows)
    finally:
        if args.json:
            with open(args.json, "w") as fh:
                json.dump(rows, fh, indent=1)
