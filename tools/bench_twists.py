"""Symmetry views (twists) measured: the view kernel beside the plain dense observation, and what views buy a deterministic search.
  1. `VecEnv.observe_twisted` (packed observation + `qg_twist_expand_packed`) at CliffordGym 16q x 65 536 in bf16 beside `observe_as(bf16)` on the
     same handle -- the untwisted path, which writes the same bytes -- alternating, graph replays on device events; written bytes over time.
  2. The reference's trained policies (tests/golden/policies) on 1 024 targets: greedy and beam_width=4 with twists=None against all views, and
     beam_width=4*V without twists -- the same batch spent on width instead of views: solved, mean gates, wall time per solve.
A record, not a gate.  Run on the GPU box: python tools/bench_twists.py [--targets 1024] [--envs 65536]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_reference_policies import MODELS, load  # noqa: E402
from util import line_gateset  # noqa: E402

import qiskit_gym_amd.envs as envs  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402
from qiskit_gym_amd.vec import VecEnv  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}


def view_kernel(B: int, reps: int = 200, windows: int = 7):
    n = 16
    vec = VecEnv("clifford", n, line_gateset("clifford", n), B, add_inverts=False, add_perms=True, track_solution=False, difficulty=64)
    vec.reset(1)
    K = vec.num_twists
    obs = 4 * n * n
    tw = (torch.arange(B, device="cuda", dtype=torch.int32) % K).contiguous()  # every twist in every wave
    out = torch.empty((B, obs), dtype=torch.bfloat16, device="cuda")
    fns = {"observe_as(bf16)": lambda: vec.observe_as(torch.bfloat16, out=out), "observe_twisted(bf16)": lambda: vec.observe_twisted(tw, torch.bfloat16, out=out)}
    graphs = {}
    for k, fn in fns.items():
        fn()  # warm-up; the first view uploads the table
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[k] = g
    plain = vec.observe_as(torch.bfloat16).clone()
    perms = torch.as_tensor(vec.twists()[0], device="cuda")
    same = bool(torch.equal(vec.observe_twisted(tw, torch.bfloat16), torch.gather(plain, 1, perms[tw.long()])))
    times = {k: [] for k in fns}
    for _ in range(windows):  # alternate the two
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    written = B * obs * 2
    for k, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        print(f"CliffordGym {n}q x {B} envs, {K} twists, {k}: {med:.1f} us per call (median of {windows} windows of {reps} graph-replayed calls, "
              f"min {ts[0]:.1f}, max {ts[-1]:.1f}); {written / 1e6:.1f} MB written -> {written / med / 1e6:.2f} TB/s = "
              f"{100.0 * written / med / 1e6 / 8.0:.0f} % of 8 TB/s", flush=True)
    print(f"view equals torch.gather of the plain observation: {same}", flush=True)
    del graphs
    vec.close()


def search_table(M: int, difficulty: int):
    for name in ("clifford_3q_custom", "lf_5_line", "perm_square_3x3"):
        cfg, gateset, w = load(name)
        kind = MODELS[name]
        gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
        syn = BatchedSynthesis(gym, policy_from_reference_state_dict(w), seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)  # targets: random scrambles made on the device, read back in the set_state wire format
        states = v.get_state("i64").cpu().numpy()
        v.close()
        syn.solve(states[:4], deterministic=True, twists=64)
        V = syn.last_stats["views"]
        runs = [("greedy, twists=None", dict(deterministic=True)), (f"greedy, twists={V}", dict(deterministic=True, twists=V)),
                ("beam_width=4, twists=None", dict(beam_width=4)), (f"beam_width=4, twists={V}", dict(beam_width=4, twists=V))]
        if 4 * V <= 64 and V > 1:
            runs.append((f"beam_width={4 * V}, twists=None", dict(beam_width=4 * V)))
        for label, kw in runs:
            syn.solve(states, **kw)  # warm-up: the handles of this batch shape
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                syn.solve(states, **kw)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            st = syn.last_stats
            print(f"{name} x {M} targets (scrambles of {difficulty} gates), {V} views available, {label}: solved {st['solved']}/{M}, "
                  f"mean gates {st['mean_gates']:.3f}, {st['steps']} steps, {best * 1e3:.1f} ms per solve (best of 3)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=32)
    ap.add_argument("--envs", type=int, default=65536)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    view_kernel(args.envs)
    search_table(args.targets, args.difficulty)
