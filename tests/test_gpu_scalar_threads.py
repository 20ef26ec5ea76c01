"""The scalar `Env` trait under host threads, as INTEGRATION.md has twisterl's workers use it: per episode clone(); reset();
loop { observe(); masks(); step(); reward(); is_final() }, the finished env dropped into the clone pool for whichever thread clones next.

Every episode's inputs are a function of (configuration, worker, episode), never of the interleaving (tests/scalar_episodes.py); the
workers only record, and after the join every transcript is replayed on a fresh CPU-oracle env and compared field by field.  Python threads
overlap inside the library (ctypes drops the GIL for each call); the compiled host of the second test has no GIL at all and a thread that
empties the pool under the workers.  The last test runs two batched handles on two threads and two streams."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import scalar_episodes as se  # noqa: E402
from oracle import OracleVec  # noqa: E402
from util import f32_bits, rng_actions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS, EPISODES = 8, 10
FAILING = (2, 5)  # the workers that also make calls that must fail
JOIN_SECONDS = 60
QG_ERR_INVALID = -1
SPECS = {s.name: s for s in se.specs()}


def _join(threads):
    for t in threads:
        t.join(JOIN_SECONDS)
    for t in threads:
        assert not t.is_alive(), f"{t.name} did not finish: a deadlock in the library"


def _endings_are_mixed(spec, endings):
    n = len(endings)
    assert "open" not in endings, "an episode of max_depth steps is final"
    if spec.kind == "pauli":
        assert endings.count("success") and endings.count("depth"), (spec.name, endings.count("success"))
    else:
        assert endings.count("success") * 4 >= n and endings.count("depth") * 4 >= n, (spec.name, endings.count("success"), n)


@pytest.mark.parametrize("name", list(SPECS))
def test_threaded_episodes_replay_on_the_oracle(name):
    from qiskit_gym_amd.envs.raw import RawEnv

    spec = SPECS[name]
    RawEnv.release_pool()  # every pooled handle of this run was parked by one of its workers
    proto = spec.raw_env(seed=1)
    transcripts, errors = {}, []

    def worker(w):
        try:
            for ep in range(EPISODES):
                transcripts[(w, ep)] = se.run_episode(spec, proto, w, ep, fail_calls=w in FAILING)
        except BaseException as err:  # reported by the main thread
            errors.append((w, repr(err)))

    threads = [threading.Thread(target=worker, args=(w,), name=f"{name}-worker-{w}", daemon=True) for w in range(WORKERS)]
    for t in threads:
        t.start()
    _join(threads)
    assert not errors, errors
    assert sorted(transcripts) == [(w, ep) for w in range(WORKERS) for ep in range(EPISODES)]
    endings = [se.replay(spec, w, ep, transcripts[(w, ep)]) for w in range(WORKERS) for ep in range(EPISODES)]
    _endings_are_mixed(spec, endings)
    # the failing calls: each thread read its own message, and (the replay above) nobody's successful calls noticed
    for w in range(WORKERS):
        failures = [f for ep in range(EPISODES) for f in transcripts[(w, ep)]["failures"]]
        assert bool(failures) == (w in FAILING)
        for what, status, message, handle in failures:
            assert status == QG_ERR_INVALID, (w, what, status, message)
            if what == "clone":
                assert message == "null argument" and handle is None, (w, message, handle)
            else:
                assert message.startswith("set_state: 3 elements per env"), (w, message)
        if w in FAILING and spec.kind != "pauli":
            assert {f[0] for f in failures} == {"clone", "set_state"}
    del proto
    RawEnv.release_pool()


HOST_SRC = r'''
/* twisterl's collection pattern from a compiled host: THREADS workers clone one prototype per episode while another thread empties the pool */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "qgym.h"
enum { THREADS = N_THREADS, EPISODES = N_EPISODES, DIFF = N_DIFF, DEPTH = N_DEPTH, OBS = 64 };
static const qg_gate gates[] = { GATES };
static const int inverse[] = { INVERSE };
enum { A = sizeof gates / sizeof gates[0] };
static qg_env *proto;
static FILE *out;
static pthread_mutex_t out_lock = PTHREAD_MUTEX_INITIALIZER;
static int stop_clearing, failed;

static int fail(const char *what, int thread, int ep) {
    fprintf(stderr, "thread %d episode %d: %s: %s\n", thread, ep, what, qg_last_error());
    __atomic_store_n(&failed, 1, __ATOMIC_SEQ_CST);
    return 1;
}
static void put(const char *line) {
    pthread_mutex_lock(&out_lock);
    fputs(line, out);
    pthread_mutex_unlock(&out_lock);
}
static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
/* draw t of env 0 of qg_env_reset(seed): the counter RNG qgym.h documents, scaled to the action count */
static int reset_draw(uint64_t seed, uint64_t t) {
    const uint64_t d = splitmix64(seed ^ splitmix64(t)), a = (uint64_t)A;
    return (int)(((d >> 32) * a + (((d & 0xFFFFFFFFull) * a) >> 32)) >> 32);
}
static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static int emit(int thread, int ep, int step, long long action, int coin, qg_env *e) {
    int64_t obs[OBS], n = qg_env_observe(e, obs, OBS), i, nm;
    uint8_t mask[A];
    uint64_t bits = 0;
    int open = 0;
    union { float f; uint32_t u; } r;
    char line[160];
    if (n < 0 || n > OBS) return fail("observe", thread, ep);
    for (i = 0; i < n; ++i) bits |= 1ull << obs[i];
    nm = qg_env_masks(e, mask, A);
    if (nm != A) return fail("masks", thread, ep);
    for (i = 0; i < A; ++i) open += mask[i] != 0;
    r.f = qg_env_reward(e);
    snprintf(line, sizeof line, "T %d %d %d %lld %d %u %d %d %d %016llx\n", thread, ep, step, action, coin, (unsigned)r.u, qg_env_is_final(e),
             qg_env_success(e), open, (unsigned long long)bits);
    put(line);
    return 0;
}

static int episode(int thread, int ep) {
    const uint64_t reset_seed = 7000u + 64u * (unsigned)thread + (unsigned)ep;
    uint32_t s = 12345u + 1000u * (unsigned)thread + (unsigned)ep;
    long long acts[DEPTH];
    int coins[DEPTH], t;
    qg_env *e = NULL;
    uint64_t sol[DEPTH + 4];
    char line[64 + 24 * (DEPTH + 4)];
    int64_t n, i;
    int len;
    for (t = 0; t < DEPTH; ++t) {
        const uint32_t a = lcg(&s) % (uint32_t)A, c = lcg(&s) & 1u, wild = lcg(&s) % 6u;
        acts[t] = a;
        coins[t] = (int)c;
        if (ep % 2 && wild == 0) acts[t] = A;   /* out of range: no gate, the depth still goes down */
        if (ep % 2 && wild == 1) acts[t] = -1;
    }
    if (ep % 2 == 0)   /* undo the scramble: the reset's draws, inverted, last gate first, no inversion coin */
        for (t = 0; t < DIFF; ++t) {
            acts[t] = inverse[reset_draw(reset_seed, (uint64_t)(DIFF - 1 - t))];
            coins[t] = 0;
        }
    if (qg_env_clone(proto, &e) != QG_OK) return fail("clone", thread, ep);
    if (qg_env_set_seed(e, reset_seed ^ 0xC10Eu) != QG_OK) return fail("set_seed", thread, ep);
    if (qg_env_reset(e, reset_seed) != QG_OK) return fail("reset", thread, ep);
    if (emit(thread, ep, 0, -9, 0, e)) return 1;
    for (t = 0; t < DEPTH && !qg_env_is_final(e); ++t) {
        if (qg_env_step_coin(e, acts[t], coins[t]) != QG_OK) return fail("step", thread, ep);
        if (emit(thread, ep, t + 1, acts[t], coins[t], e)) return 1;
    }
    n = qg_env_solution(e, sol, DEPTH + 4);
    if (n < 0 || n > DEPTH + 4) return fail("solution", thread, ep);
    len = snprintf(line, sizeof line, "S %d %d", thread, ep);
    for (i = 0; i < n; ++i) len += snprintf(line + len, sizeof line - (size_t)len, " %llu", (unsigned long long)sol[i]);
    snprintf(line + len, sizeof line - (size_t)len, "\n");
    put(line);
    qg_env_destroy(e);   /* into the pool: the next clone, on whichever thread, takes it out */
    return 0;
}

static void *worker(void *arg) {
    const int thread = (int)(size_t)arg;
    int ep;
    for (ep = 0; ep < EPISODES; ++ep)
        if (episode(thread, ep)) break;
    return NULL;
}
static void *clearer(void *arg) {
    const struct timespec nap = {0, 2000000};   /* 2 ms */
    (void)arg;
    while (!__atomic_load_n(&stop_clearing, __ATOMIC_SEQ_CST)) {
        qg_env_pool_clear();
        nanosleep(&nap, NULL);
    }
    return NULL;
}

int main(int argc, char **argv) {
    pthread_t workers[THREADS], clear_thread;
    qg_config cfg;
    size_t i;
    if (argc != 2 || !(out = fopen(argv[1], "w"))) return 2;
    qg_config_default(&cfg, QG_CLIFFORD, 4);   /* add_inverts and track_solution are on */
    cfg.add_perms = 0;
    cfg.difficulty = DIFF;
    cfg.max_depth = DEPTH;
    if (qg_env_create(&cfg, gates, A, 0, &proto) != QG_OK) return fail("create", -1, -1) + 9;
    if (pthread_create(&clear_thread, NULL, clearer, NULL)) return 3;
    for (i = 0; i < THREADS; ++i)
        if (pthread_create(&workers[i], NULL, worker, (void *)i)) return 3;
    for (i = 0; i < THREADS; ++i) pthread_join(workers[i], NULL);
    __atomic_store_n(&stop_clearing, 1, __ATOMIC_SEQ_CST);
    pthread_join(clear_thread, NULL);
    if (!failed) episode(THREADS, 0);   /* after all that: one more clone of the prototype, stepped */
    qg_env_destroy(proto);
    qg_env_pool_clear();
    fclose(out);
    return failed ? 10 : 0;
}
'''


def _lcg_plan(spec, thread, ep, reset_seed):
    """HOST_SRC's episode() inputs, restated."""
    s = (12345 + 1000 * thread + ep) & 0xFFFFFFFF
    acts, coins = [], []

    def lcg():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        return s >> 8

    for t in range(spec.max_depth):
        a, c, wild = lcg() % spec.A, lcg() & 1, lcg() % 6
        if ep % 2 and wild == 0:
            a = spec.A
        if ep % 2 and wild == 1:
            a = -1
        acts.append(a)
        coins.append(c)
    if ep % 2 == 0:
        draws = rng_actions(reset_seed, [0], spec.difficulty, spec.A)[:, 0]
        for t in range(spec.difficulty):
            acts[t], coins[t] = spec.inverse[int(draws[spec.difficulty - 1 - t])], 0
    return acts, coins


def test_compiled_host_threads_share_the_pool_while_it_is_cleared(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.envs.gateset import parse_gateset

    spec = SPECS["clifford4-defaults"]
    threads, episodes = 16, 24
    src = HOST_SRC
    for key, val in (("N_THREADS", threads), ("N_EPISODES", episodes), ("N_DIFF", spec.difficulty), ("N_DEPTH", spec.max_depth),
                     ("GATES", ", ".join("{%d, %d, %d}" % g for g in parse_gateset(spec.gateset))), ("INVERSE", ", ".join(map(str, spec.inverse)))):
        src = src.replace(key, str(val))
    (tmp_path / "host.c").write_text(src)
    _lib.load()
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "qiskit_gym_amd", "lib")
    exe, log = tmp_path / "host", tmp_path / "transcripts.txt"
    subprocess.run(["gcc", "-std=c99", "-pthread", "-Wall", "-I", inc, str(tmp_path / "host.c"), "-o", str(exe), "-L", libdir, "-lqgym",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=120)
    out = subprocess.run([str(exe), str(log)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    steps, solutions = {}, {}
    for ln in log.read_text().splitlines():
        f = ln.split()
        if f[0] == "T":
            steps.setdefault((int(f[1]), int(f[2])), {})[int(f[3])] = (int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]), int(f[10], 16))
        else:
            assert f[0] == "S" and (int(f[1]), int(f[2])) not in solutions
            solutions[(int(f[1]), int(f[2]))] = [int(x) for x in f[3:]]
    want_keys = [(t, ep) for t in range(threads) for ep in range(episodes)] + [(threads, 0)]
    assert sorted(steps) == want_keys and sorted(solutions) == want_keys
    endings = []
    for thread, ep in want_keys:
        reset_seed = 7000 + 64 * thread + ep
        acts, coins = _lcg_plan(spec, thread, ep, reset_seed)
        ora = spec.oracle_env()
        se.oracle_reset(spec, ora, reset_seed)
        got = steps[(thread, ep)]
        t = 0
        while True:
            obs, mask, reward, final, success = se.oracle_frame(ora)
            want = (-9 if t == 0 else acts[t - 1], 0 if t == 0 else coins[t - 1], reward, int(final), int(success), sum(mask), sum(1 << i for i in obs))
            assert got.get(t) == want, (thread, ep, t, got.get(t), want)
            if final or t == spec.max_depth:
                break
            ora.step(acts[t], coins[t])
            t += 1
        assert len(got) == t + 1, (thread, ep, "the program stepped a final env")
        assert solutions[(thread, ep)] == ora.solution(), (thread, ep)
        endings.append("success" if success else "depth" if final else "open")
    _endings_are_mixed(spec, endings)


def test_two_batched_handles_on_two_threads_and_streams():
    """Nothing process-wide (the per-thread event pool, the compute-unit cache, scratch) is shared between handles in a way that matters: two
    VecEnvs, each built and driven by its own thread under its own stream -- reset, 12 steps, reset_done, 12 steps -- against OracleVec."""
    from qiskit_gym_amd.vec import VecEnv

    T = 12
    cases = [("clifford", 16, 4097, 11), ("linear_function", 8, 8192, 12)]
    runs, errors = {}, []
    for kind, n, B, seed in cases:
        spec = se.Spec(kind, kind, n, se.line_gateset(kind, n), add_inverts=False, add_perms=False, track_solution=False, difficulty=2, depth_slope=8,
                       max_depth=16)  # (16 steps to an episode)
        rng = np.random.default_rng(seed)
        acts = rng.integers(0, spec.A, size=(2 * T, B))
        acts[::5, 1::7] = -1
        # every third env idles (out of range: no gate, the depth goes down) and then undoes its scramble, so that the step before
        # reset_done leaves it solved; the others are mid-episode there
        draws = rng_actions(seed, B, 2, spec.A)
        acts[:T - 2, ::3] = spec.A
        acts[T - 2, ::3] = np.asarray(spec.inverse)[draws[1, ::3]]
        acts[T - 1, ::3] = np.asarray(spec.inverse)[draws[0, ::3]]
        runs[kind] = dict(spec=spec, B=B, seed=seed, acts=acts, got=[])

    def drive(kind):
        run = runs[kind]
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                spec = run["spec"]
                gv = VecEnv(spec.kind, spec.n, spec.gateset, run["B"], **spec.cfg)
                acts = torch.as_tensor(run["acts"], device="cuda", dtype=torch.int32)
                gv.reset(run["seed"])
                for t in range(2 * T):
                    if t == T:
                        gv.reset_done(run["seed"] + 100)
                    gv.step(acts[t])
                    gv.sync()
                    run["got"].append((gv.reward.cpu().numpy(), gv.success.cpu().numpy(), gv.done.cpu().numpy(), gv.depth.cpu().numpy()))
                    if t in (T - 1, 2 * T - 1):
                        run["got"].append(gv.observe().cpu().numpy().reshape(run["B"], -1))
                gv.close()
        except BaseException as err:
            errors.append((kind, repr(err)))

    threads = [threading.Thread(target=drive, args=(kind,), name=f"vec-{kind}", daemon=True) for kind in runs]
    for t in threads:
        t.start()
    _join(threads)
    assert not errors, errors
    for kind, run in runs.items():
        ov = OracleVec(run["spec"].oracle_env(), run["B"])
        ov.reset_seeded(run["seed"])
        got = iter(run["got"])
        final = None
        for t in range(2 * T):
            if t == T:
                assert 0 < final.sum() < run["B"] and final[::3].all(), "reset_done has some envs to reset and some to leave"
                ov.reset_seeded(run["seed"] + 100, mask=final)
            reward, success, final, depth = ov.step(run["acts"][t])
            g_reward, g_success, g_done, g_depth = next(got)
            np.testing.assert_array_equal(f32_bits(g_reward), f32_bits(reward), err_msg=f"{kind} reward t={t}")
            np.testing.assert_array_equal(g_success, success, err_msg=f"{kind} success t={t}")
            np.testing.assert_array_equal(g_done, final, err_msg=f"{kind} is_final t={t}")
            np.testing.assert_array_equal(g_depth, depth, err_msg=f"{kind} depth t={t}")
            if t in (T - 1, 2 * T - 1):
                np.testing.assert_array_equal(next(got), ov.observe_dense(), err_msg=f"{kind} observation t={t}")
