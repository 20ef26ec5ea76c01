"""Beam search beside the sampled and the greedy search of BatchedSynthesis, with the reference's trained policies (tests/golden/policies):
solved targets and mean gate count for beam_width 1 / 4 / 16, deterministic=True and num_searches=16 on the same targets; then the time of
the selection kernel (`collector.beam_select`) beside the torch expression it replaces, alternating, on device events.  A record, not a gate.
--merge: instead, beam_width 4 / 16 / 64 with and without merge_duplicates on the same targets: solved, mean gates, time per solve and the share
of the live beams that the merge drops (revisits and duplicates apart); under `rocprofv3 --kernel-trace --stats` the same run gives
beam_merge_kernel beside beam_select_kernel and copy_envs_kernel.
--bound: instead, bound=None / "stop" / "prune" in one process on the same targets -- the three trained policies and CliffordGym 16q under a seeded
random policy, beam_width 1 / 4 / 16, with and without merge_duplicates, clifford_3q_custom once more with fast=True: solved, mean gates, steps,
beams ended by the bound, time per solve (the three bounds alternate, best of the windows); then the `collector.beam_advance` launch beside the
tensor-library lines of the search that it replaces.
Run on the GPU box: python tools/bench_beam.py [--targets 1024] [--merge [--widths 4 16 64] | --bound [--widths 1 4 16]]"""
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
from qiskit_gym_amd.collector import BasicPolicy, beam_advance, beam_select  # noqa: E402
from qiskit_gym_amd.envs.gateset import gateset_from_coupling_map, line_edges  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}


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
        runs = [("deterministic=True", dict(deterministic=True)), ("num_searches=16", dict(num_searches=16))]
        runs += [(f"beam_width={W}", dict(beam_width=W)) for W in (1, 4, 16)]
        for label, kw in runs:
            syn.solve(states[:8], **kw)  # warm-up (library handles, the handles of this batch shape are built in the timed call)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            syn.solve(states, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = syn.last_stats
            print(f"{name} x {M} targets (scrambles of {difficulty} gates), {label}: solved {st['solved']}/{M}, mean gates {st['mean_gates']:.2f}, "
                  f"{st['steps']} steps, {dt * 1e3:.1f} ms incl. handle creation", flush=True)


def merge_table(M: int, difficulty: int, widths):
    import qiskit_gym_amd.synthesis as synthesis

    for name in ("clifford_3q_custom", "lf_5_line", "perm_square_3x3"):
        cfg, gateset, w = load(name)
        kind = MODELS[name]
        gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
        syn = BatchedSynthesis(gym, policy_from_reference_state_dict(w), seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)
        states = v.get_state("i64").cpu().numpy()
        v.close()
        for W in widths:
            for merge in (False, True):
                kw = dict(beam_width=W, merge_duplicates=merge)
                syn.solve(states, **kw)  # warm-up: the handles of this batch shape
                torch.cuda.synchronize()
                best = float("inf")
                for _ in range(3):
                    t0 = time.perf_counter()
                    syn.solve(states, **kw)
                    torch.cuda.synchronize()
                    best = min(best, time.perf_counter() - t0)
                st = syn.last_stats
                line = (f"{name} x {M} targets (scrambles of {difficulty} gates), beam_width={W}, merge_duplicates={merge}: solved {st['solved']}/{M}, "
                        f"mean gates {st['mean_gates']:.3f}, {st['steps']} steps, {best * 1e3:.1f} ms per solve (best of 3)")
                if merge:  # once more, untimed, counting the live beams every merge call is given (the first call holds the targets alone)
                    seen_live, real = [], synthesis.beam_merge

                    def counting(words, cum, live, *a, **k):
                        seen_live.append(live.sum())
                        return real(words, cum, live, *a, **k)

                    synthesis.beam_merge = counting
                    try:
                        syn.solve(states, **kw)
                    finally:
                        synthesis.beam_merge = real
                    offered = int(torch.stack(seen_live[1:]).sum())
                    line += (f"; of {offered} live beams offered to the merge {syn.last_stats['revisits']} ({100.0 * syn.last_stats['revisits'] / max(1, offered):.1f} %) "
                             f"were revisits, {syn.last_stats['merged']} ({100.0 * syn.last_stats['merged'] / max(1, offered):.1f} %) duplicates")
                print(line, flush=True)


def torch_select(logp, cum, live, W, A):
    """The tensor-library expression of the same selection (without the tie rule: topk's order among equal scores is unspecified)."""
    B = logp.shape[0]
    M = B // W
    score = torch.where(live.bool()[:, None], cum[:, None] + logp[:, :A].float(), torch.full((), -float("inf"), device=logp.device)).view(M, W * A)
    val, idx = score.topk(W, dim=1)
    ok = val > -float("inf")
    slot = idx // A
    base = torch.arange(M, device=logp.device)[:, None] * W
    own = base + torch.arange(W, device=logp.device)[None, :]
    parent = torch.where(ok, base + slot, own).to(torch.int32).view(B)
    act = torch.where(ok, idx - slot * A, torch.full_like(idx, A)).to(torch.int32).view(B)
    return parent, act, val.reshape(B), ok.to(torch.uint8).view(B)


def select_times(reps: int = 200):
    for M, W, A in ((1024, 16, 27), (1024, 16, 170), (1024, 64, 170), (4096, 16, 170), (64, 64, 222)):
        B = M * W
        g = torch.Generator(device="cuda").manual_seed(M + W + A)
        logp = torch.log_softmax(torch.randn((B, A), device="cuda", generator=g), dim=1)
        cum = -torch.rand(B, device="cuda", generator=g) * 5
        live = (torch.rand(B, device="cuda", generator=g) < 0.9).to(torch.uint8)
        a, b = beam_select(logp, cum, live, W, A), torch_select(logp, cum, live, W, A)
        torch.cuda.synchronize()
        same = all(bool((x.to(torch.float32) == y.to(torch.float32)).all()) for x, y in zip(a, b))  # continuous scores: no ties
        fns = {"beam_select": lambda: beam_select(logp, cum, live, W, A), "torch topk": lambda: torch_select(logp, cum, live, W, A)}
        best = {k: float("inf") for k in fns}
        for _ in range(5):  # alternate the two; the best of five windows each
            for k, fn in fns.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best[k] = min(best[k], e0.elapsed_time(e1) * 1e3 / reps)
        print(f"select {M} targets x {W} beams x {A} actions (f32, eager, {reps} calls per window): beam_select {best['beam_select']:.1f} us, "
              f"torch expression {best['torch topk']:.1f} us per call; same result: {same}", flush=True)


def bound_table(M: int, difficulty: int, widths, reps: int = 3):
    cases = []
    for name in ("clifford_3q_custom", "lf_5_line", "perm_square_3x3"):
        cfg, gateset, w = load(name)
        gym = getattr(envs, GYMS[MODELS[name]])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
        cases.append((name, gym, policy_from_reference_state_dict(w), (False,) if name != "clifford_3q_custom" else (False, True)))
    n, gs = gateset_from_coupling_map(line_edges(16, True), None, ["H", "S", "Sdg", "SX", "SXdg", "CX", "CZ", "SWAP"])
    torch.manual_seed(16)
    cases.append(("CliffordGym 16q (random policy, max_depth 40)", envs.CliffordGym(n, gs, max_depth=40), BasicPolicy(4 * n * n, len(gs)), (False,)))
    for name, gym, policy, fasts in cases:
        syn = BatchedSynthesis(gym, policy, seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)
        states = v.get_state("i64").cpu().numpy()
        v.close()
        for fast in fasts:
            for W in widths:
                for merge in (False, True):
                    kws = {b: dict(beam_width=W, merge_duplicates=merge, bound=b, fast=True if fast else None) for b in (None, "stop", "prune")}
                    best, stats, sols = {b: float("inf") for b in kws}, {}, {}
                    for kw in kws.values():
                        syn.solve(states, **kw)  # warm-up: the handles of this batch shape, every code path
                    torch.cuda.synchronize()
                    for _ in range(reps):  # the three alternate
                        for b, kw in kws.items():
                            t0 = time.perf_counter()
                            sols[b] = syn.solve(states, **kw)
                            torch.cuda.synchronize()
                            best[b] = min(best[b], time.perf_counter() - t0)
                            stats[b] = dict(syn.last_stats)
                    for b in kws:
                        st = stats[b]
                        same = "" if b is None else f", solutions equal to bound=None: {sols[b] == sols[None]}"
                        print(f"{name} x {M} targets (scrambles of {difficulty} gates), beam_width={W}, merge_duplicates={merge}, fast={fast}, bound={b}: "
                              f"solved {st['solved']}/{M}, mean gates {st['mean_gates']:.3f}, {st['steps']} steps, bounded {st.get('bounded', '-')}, "
                              f"{best[b] * 1e3:.1f} ms per solve (best of {reps}), {best[b] * 1e6 / max(1, st['steps']):.0f} us per step{same}", flush=True)


def torch_advance(parent, ret, reward, success, done, live, best, found, W, group, nowhere):
    """The lines that `BatchedSynthesis._beam_search` ran for bound=None before `beam_advance` took their place, up to the source index of the
    winners' copy: the record of what the launch replaced."""
    M = best.shape[0]
    ret = ret[parent.long()] + reward
    solved = (live.bool() & success.bool()).view(M, W)
    live = live & (1 - done)
    score = torch.where(solved, ret.view(M, W), torch.full((M, W), -float("inf"), device=ret.device))
    j = score.argmax(dim=1)
    val = score.gather(1, j.view(M, 1)).view(M)
    better = val > best
    src = torch.where(better, group * W + j.to(torch.int32), nowhere)
    return ret, live, torch.where(better, val, best), found | better, src


def advance_times(reps: int = 200):
    for M, W in ((1024, 4), (1024, 16), (4096, 16)):
        B = M * W
        g = torch.Generator(device="cuda").manual_seed(M + W)
        parent = (torch.arange(B, device="cuda") // W * W + torch.randint(0, W, (B,), device="cuda", generator=g)).to(torch.int32)
        ret, reward = -torch.rand(B, device="cuda", generator=g), -torch.rand(B, device="cuda", generator=g) * 0.02
        success = (torch.rand(B, device="cuda", generator=g) < 0.05).to(torch.uint8)
        reward += success
        live0 = (torch.rand(B, device="cuda", generator=g) < 0.9).to(torch.uint8)
        best0, found0 = torch.full((M,), -float("inf"), device="cuda"), torch.zeros(M, dtype=torch.bool, device="cuda")
        group, nowhere = torch.arange(M, dtype=torch.int32, device="cuda"), torch.full((M,), B, dtype=torch.int32, device="cuda")
        live, best, found = live0.clone(), best0.clone(), found0.clone()
        out = dict(ret_out=torch.empty(B, device="cuda"), win_src=torch.empty(M, dtype=torch.int32, device="cuda"),
                   group_live=torch.empty(M, dtype=torch.uint8, device="cuda"), bounded=torch.zeros(M, dtype=torch.int32, device="cuda"))

        def kernel(mode):  # live, best and found are updated in place: from the second call on they are their own fixed point, the work is the same
            return beam_advance(parent, ret, reward, success, success, live, best, found, W, B, 1.0, mode, **out)

        def lines():
            return torch_advance(parent, ret, reward, success, success, live0, best0, found0, W, group, nowhere)

        t = lines()
        k = kernel(None)
        torch.cuda.synchronize()
        on = live0.bool()
        same = bool((k[0][on] == t[0][on]).all()) and bool((live == t[1]).all()) and bool((best == t[2]).all()) and bool((found == t[3]).all()) and bool((k[1] == t[4]).all())
        fns = {"beam_advance": lambda: kernel(None), "beam_advance stop": lambda: kernel("stop"), "torch lines": lines}
        times = {k_: float("inf") for k_ in fns}
        for _ in range(5):  # alternate; the best of five windows each
            for k_, fn in fns.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k_] = min(times[k_], e0.elapsed_time(e1) * 1e3 / reps)
        print(f"advance {M} targets x {W} beams (eager, the launch alone, {reps} calls per window): "
              f"beam_advance {times['beam_advance']:.1f} us, with mode stop {times['beam_advance stop']:.1f} us, torch lines {times['torch lines']:.1f} us per call; "
              f"same result: {same}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=32)
    ap.add_argument("--merge", action="store_true", help="the merge_duplicates table instead of the search table and the selection times")
    ap.add_argument("--bound", action="store_true", help="the bound table (None / stop / prune) and the beam_advance launch beside the torch lines instead")
    ap.add_argument("--widths", type=int, nargs="+", default=None, help="default: 4 16 64 with --merge, 1 4 16 with --bound")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if args.bound:
        bound_table(args.targets, args.difficulty, args.widths or [1, 4, 16])
        advance_times()
    elif args.merge:
        merge_table(args.targets, args.difficulty, args.widths or [4, 16, 64])
    else:
        search_table(args.targets, args.difficulty)
        select_times()
