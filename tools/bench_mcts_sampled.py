"""The sampled tree search of BatchedSynthesis, `solve(num_searches=S, num_mcts_searches=N, mcts_sampled=True)`, with the reference's trained
policies (tests/golden/policies), beside the deterministic tree search at the same N, the policy-sampled search at num_searches=64 and beam 4
on the same targets, in one process: solved targets, mean gates, decisions and time per solve (every call made twice, the second timed: a host
clock around a solve that ends in a synchronise); every 8th answer of the sampled tree searches is replayed on the oracle.  Then the
`collector.mcts_decide` launch, in both modes, beside the tensor-library lines of the deterministic search's decision that it restates, on
forests driven with random rows, alternating, on device events.  Then what the forest and the pool of node envs take.  A record, not a gate.
Run on the GPU box: python tools/bench_mcts_sampled.py [--targets 1024] [--difficulty 20] [--skip-search]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_reference_policies import MODELS, load  # noqa: E402

import qiskit_gym_amd.envs as envs  # noqa: E402
from qiskit_gym_amd import _lib  # noqa: E402
from qiskit_gym_amd.collector import mcts_backup, mcts_decide, mcts_forest, mcts_select  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}
NAMES = ("clifford_3q_custom", "lf_5_line", "perm_square_3x3")
SHAPES = ((8, 8), (8, 32))  # (S, N)


def gym_of(name):
    cfg, gateset, w = load(name)
    kind = MODELS[name]
    gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    return kind, cfg, gateset, gym, policy_from_reference_state_dict(w)


def search_table(M: int, difficulty: int):
    from test_gpu_synthesis import replay

    for name in NAMES:
        kind, cfg, gateset, gym, policy = gym_of(name)
        syn = BatchedSynthesis(gym, policy, seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)  # targets: random scrambles made on the device, read back in the set_state wire format
        states = v.get_state("i64").cpu().numpy()
        v.close()
        runs = [("deterministic=True", dict(deterministic=True)), ("num_searches=64", dict(num_searches=64)), ("beam_width=4", dict(beam_width=4))]
        for S, N in SHAPES:
            runs.append((f"deterministic=True, num_mcts_searches={N}", dict(deterministic=True, num_mcts_searches=N)))
            runs.append((f"num_searches={S}, num_mcts_searches={N}, mcts_sampled=True", dict(num_searches=S, num_mcts_searches=N, mcts_sampled=True)))
        for label, kw in runs:
            syn.solve(states, **kw)  # the handles of this batch shape, every code path
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sols = syn.solve(states, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = syn.last_stats
            extra = ""
            if kw.get("mcts_sampled"):
                rcfg = dict(num_qubits=cfg["num_qubits"], depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
                checked = [replay(kind, rcfg, gateset, states[m].tolist(), sols[m]).success() for m in range(0, M, 8) if sols[m] is not None]
                extra = f", searches solved {st['searches_solved']:.4f}, {sum(checked)} of {len(checked)} replayed answers solve their target"
            if "nodes" in st:
                extra += f", mean nodes per tree {st['nodes']:.2f}"
            print(f"{name} x {M} targets (scrambles of {difficulty} gates), {label}: solved {st['solved']}/{M}, mean gates {st['mean_gates']:.3f}, "
                  f"{st['steps']} steps, {dt * 1e3:.1f} ms per solve{extra}", flush=True)


def torch_decide(forest, finished, keys, parked):
    """The tensor-library lines with which the plain deterministic search took its decision before every mode went to `mcts_decide`: kept
    as the historical comparison."""
    A = forest.A
    child = forest.child[:, 0, :].to(torch.int64)
    visits = torch.gather(forest.visits.to(torch.int64), 1, child.clamp(min=0))
    best = torch.where(child >= 0, visits * A + keys, -1).max(dim=1).values
    return torch.where((best >= 0) & (finished == 0), A - 1 - best % A, parked).to(torch.int32)


def decide_times(reps: int = 200):
    for M, N, A in ((1024, 32, 170), (8192, 32, 170)):
        g = torch.Generator(device="cuda").manual_seed(M + N + A)
        forest = mcts_forest(M, N, A, "cuda")

        def rows():
            return (torch.log_softmax(torch.randn((M, A), device="cuda", generator=g), dim=1), torch.randn(M, device="cuda", generator=g),
                    torch.rand(M, device="cuda", generator=g) - 0.5, (torch.rand(M, device="cuda", generator=g) < 0.1).to(torch.uint8))

        logp, values, _, _ = rows()
        mcts_backup(forest, logp, values, root=True)
        for _ in range(N):
            picked = mcts_select(forest, 2 ** 0.5)
            logp, values, reward, done = rows()
            mcts_backup(forest, logp, values, reward, done, *picked)
        finished = (torch.rand(M, device="cuda", generator=g) < 0.1).to(torch.uint8)
        keys = torch.arange(A - 1, -1, -1, dtype=torch.int64, device="cuda")
        parked = torch.full((M,), A, dtype=torch.int32, device="cuda")
        move, counts = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty((M, A), dtype=torch.int32, device="cuda")
        same = bool((mcts_decide(forest, finished=finished) == torch_decide(forest, finished, keys, parked)).all())
        children = float((forest.child[:, 0, :] >= 0).sum()) / M
        fns = {"most visited": lambda: mcts_decide(forest, finished=finished, move=move),
               "sample": lambda: mcts_decide(forest, sample=True, seed=1, counter=7, finished=finished, move=move),
               "sample + counts": lambda: mcts_decide(forest, sample=True, seed=1, counter=7, finished=finished, move=move, counts=counts),
               "torch lines": lambda: torch_decide(forest, finished, keys, parked)}
        best = {k: float("inf") for k in fns}
        for _ in range(5):  # alternate; the best of five windows each
            for k, fn in fns.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best[k] = min(best[k], e0.elapsed_time(e1) * 1e3 / reps)
        print(f"decide {M} trees x {A} actions after {N} simulations ({children:.1f} root children per tree; eager, the launches alone, {reps} calls per "
              f"window): " + ", ".join(f"{k} {v:.1f} us" for k, v in best.items()) + f" per call; most visited equals the torch lines: {same}", flush=True)


def memory(M: int):
    L = _lib.load()
    for name in NAMES:
        kind, cfg, gateset, gym, _ = gym_of(name)
        A = len(gateset)
        for S, N in SHAPES:
            B = M * S
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            pool = gym.vec(B * (N + 1), add_inverts=False, add_perms=False, track_solution=True)
            torch.cuda.synchronize()
            taken = free0 - torch.cuda.mem_get_info()[0]
            pool.close()
            print(f"{name} ({A} actions), {M} targets x {S} searches, N = {N}: forest {int(L.qg_mcts_forest_bytes(B, N + 1, A))} bytes, the pool of "
                  f"{B * (N + 1)} node envs took {taken} bytes of device memory", flush=True)
    per_tree = int(L.qg_mcts_forest_bytes(1, 33, 170))
    print(f"N = 32, 170 actions: {per_tree} bytes per tree, the 1 GiB forest limit admits {(1 << 30) // per_tree} trees", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=20)
    ap.add_argument("--skip-search", action="store_true", help="the launch times and the memory figures alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    decide_times()
    memory(args.targets)
    if not args.skip_search:
        search_table(args.targets, args.difficulty)
