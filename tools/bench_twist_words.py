"""Twisted searches on the policy-layer kernels, measured.
  1. The view as packed words (`VecEnv.observe_twisted_words`: packed observation + `qg_twist_pack_words`) beside the bf16 view it replaces
     (`VecEnv.observe_twisted(bf16)`) on the same handle, per-env random twists, at CliffordGym 16q x 1 024 and x 65 536 and
     LinearFunctionGym 8q x 8 192: device time per call, graph replays between device events, the two alternating.  --first-layer adds
     what follows either view: `embed_words` on the words beside a bf16 `Linear` on the dense view.
  2. `solve(twists=V, twist_kernels=True)` beside the torch path `solve(twists=V)` in the same process, the reference's trained policies
     (tests/golden/policies) on 1 024 targets, V = 2 and every view the env has, greedy / beam_width=4 / num_searches=64: time per solve,
     solved targets, mean gates.
A record, not a gate.  Run on the GPU box: python tools/bench_twist_words.py [--targets 1024] [--skip-kernel] [--skip-search]"""
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
from qiskit_gym_amd.collector import embed_words, pack_embed_words  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402
from qiskit_gym_amd.vec import VecEnv  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}


def replay_times(fns, reps: int, windows: int):
    """Median / min / max device time per call in us: every fn captured `reps` times into a graph, the graphs replayed in turn."""
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
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    del graphs
    return {k: (sorted(ts)[len(ts) // 2], min(ts), max(ts)) for k, ts in times.items()}


def view_kernel(kind: str, n: int, B: int, first_layer: bool, reps: int = 200, windows: int = 7):
    vec = VecEnv(kind, n, line_gateset(kind, n), B, add_inverts=False, add_perms=True, track_solution=False, difficulty=4 * n)
    vec.reset(1)
    K = vec.num_twists
    rows, cols = vec.obs_shape_
    rows_out = rows + rows % 2
    g = torch.Generator(device="cuda").manual_seed(B)
    tw = torch.randint(0, K, (B,), device="cuda", generator=g, dtype=torch.int32)  # every env its own twist
    dense = torch.empty((B, rows * cols), dtype=torch.bfloat16, device="cuda")
    words = torch.empty((B, rows_out), dtype=torch.int64, device="cuda")
    fns = {"observe_twisted(bf16)": lambda: vec.observe_twisted(tw, torch.bfloat16, out=dense),
           "observe_twisted_words": lambda: vec.observe_twisted_words(tw, rows_out, out=words)}
    if first_layer:
        hidden = 512
        lin = torch.nn.Linear(rows * cols, hidden, device="cuda", dtype=torch.bfloat16)
        w = lin.weight.detach()
        packed = pack_embed_words(torch.nn.functional.pad(w, (0, cols)) if rows % 2 else w, rows_out, cols)
        bias = lin.bias.detach().float().contiguous()
        h = torch.empty((B, hidden), dtype=torch.bfloat16, device="cuda")
        fns["observe_twisted(bf16) + bf16 Linear + relu"] = lambda: torch.relu_(lin(vec.observe_twisted(tw, torch.bfloat16, out=dense)))
        fns["observe_twisted_words + embed_words"] = lambda: embed_words(vec.observe_twisted_words(tw, rows_out, out=words), cols, packed, bias, hidden, relu=True, out=h)
    # the two views hold the same bits
    bits = ((vec.observe_twisted_words(tw, rows_out)[:, :rows].unsqueeze(-1) >> torch.arange(cols, device="cuda")) & 1).flatten(1)
    same = bool(torch.equal(bits.to(torch.bfloat16), vec.observe_twisted(tw, torch.bfloat16)))
    with torch.no_grad():
        res = replay_times(fns, reps, windows)
    written = {"observe_twisted(bf16)": B * rows * cols * 2, "observe_twisted_words": B * rows_out * 8}
    for k, (med, lo, hi) in res.items():
        line = (f"{kind} {n}q x {B} envs, {K} twists, {k}: {med:.1f} us per call (median of {windows} windows of {reps} graph-replayed calls, "
                f"min {lo:.1f}, max {hi:.1f})")
        if k in written:
            line += f"; {written[k] / 1e6:.2f} MB written"
        print(line, flush=True)
    print(f"{kind} {n}q x {B}: the words hold the bits of the bf16 view: {same}", flush=True)
    vec.close()


def search_table(M: int, difficulty: int, names):
    modes = [("deterministic=True", dict(deterministic=True)), ("beam_width=4", dict(beam_width=4)), ("num_searches=64", dict(num_searches=64))]
    for name in names:
        cfg, gateset, w = load(name)
        kind = MODELS[name]
        gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
        syn = BatchedSynthesis(gym, policy_from_reference_state_dict(w), seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)  # targets: random scrambles made on the device, read back in the set_state wire format
        states = v.get_state("i64").cpu().numpy()
        v.close()
        full = len(syn._views(1 << 30))
        for V in sorted({min(2, full), full}):
            for label, kw in modes:
                paths = {"torch": dict(twists=V), "kernels": dict(twists=V, twist_kernels=True)}
                best = {k: float("inf") for k in paths}
                stats = {}
                for k, extra in paths.items():
                    syn.solve(states, **kw, **extra)  # warm-up: the handles of this batch shape
                torch.cuda.synchronize()
                for _ in range(3):  # alternate the two; the best of three each
                    for k, extra in paths.items():
                        t0 = time.perf_counter()
                        syn.solve(states, **kw, **extra)
                        torch.cuda.synchronize()
                        best[k] = min(best[k], time.perf_counter() - t0)
                        stats[k] = dict(syn.last_stats)
                t, k = stats["torch"], stats["kernels"]
                print(f"{name} x {M} targets (scrambles of {difficulty} gates), {t['views']} views, {label}: torch path {best['torch'] * 1e3:.1f} ms per solve, "
                      f"solved {t['solved']}/{M}, mean gates {t['mean_gates']:.3f}, {t['steps']} steps | twist_kernels {best['kernels'] * 1e3:.1f} ms per solve, "
                      f"solved {k['solved']}/{M}, mean gates {k['mean_gates']:.3f}, {k['steps']} steps (best of 3 each)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=32)
    ap.add_argument("--policies", nargs="+", default=["clifford_3q_custom", "lf_5_line"])
    ap.add_argument("--first-layer", action="store_true", help="also time each view together with the first layer that reads it")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-search", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if not args.skip_kernel:
        for kind, n, B in (("clifford", 16, 1024), ("clifford", 16, 65536), ("linear_function", 8, 8192)):
            view_kernel(kind, n, B, args.first_layer)
    if not args.skip_search:
        search_table(args.targets, args.difficulty, args.policies)
