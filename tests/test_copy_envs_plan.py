"""qg_vec_copy_envs on the CPU: the state regions the copy kernel walks for every layout (`qg_plan_query(QG_PLAN_COPY_ENVS)`, answered from
qgym_plan.hpp copy_layout, the function the launch path calls), and DoneListState's copy transition (qgym_done_list.hpp), which must leave
a handle's list of finished envs as qg_vec_set_state leaves it."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from qiskit_gym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qiskit_gym_amd", "csrc")
COPY_ENVS = 9
PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
DEFAULT = dict(add_inverts=True, add_perms=False, track_solution=True)
LAYERS = dict(n_layers=1.0, n_layers_cnots=0.5)


def copy_plan(kind, n, batch=4096, weights=None, **cfg):
    L = _lib.load()
    c = _lib.make_config(kind, n, metrics_weights=weights, **cfg)
    buf = C.create_string_buffer(128)
    rc = L.qg_plan_query(C.byref(c), batch, 170, COPY_ENVS, 0, 0, buf, len(buf))
    return buf.value.decode() if rc == 0 else rc


ROWS = [
    # kind, qubits, options -> "rows x bytes per lane" of each region of a 64-env tile
    # TILE: R / 4 groups of four uint32 row slots (Clifford R = 2 * ceil4(N), LinearFunction R = ceil4(N))
    ("clifford", 3, PLAIN, "2x16"), ("clifford", 8, PLAIN, "4x16"), ("clifford", 16, PLAIN, "8x16"), ("clifford", 16, DEFAULT, "8x16"),
    ("linear_function", 9, PLAIN, "3x16"), ("linear_function", 16, PLAIN, "4x16"), ("linear_function", 32, PLAIN, "8x16"),
    # TILE64: two uint64 rows per group
    ("clifford", 17, PLAIN, "20x16"), ("clifford", 24, PLAIN, "24x16"), ("clifford", 32, DEFAULT, "32x16"),
    ("linear_function", 33, PLAIN, "20x16"), ("linear_function", 48, PLAIN, "24x16"), ("linear_function", 64, PLAIN, "32x16"),
    # one uint64 per env
    ("linear_function", 3, PLAIN, "1x8"), ("linear_function", 8, DEFAULT, "1x8"), ("permutation", 9, PLAIN, "1x8"), ("permutation", 16, DEFAULT, "1x8"),
    # PERMB: 16 one-byte entries per group
    ("permutation", 17, PLAIN, "2x16"), ("permutation", 100, DEFAULT, "7x16"), ("permutation", 256, PLAIN, "16x16"),
    # LFD: the matrix's groups, then the inverse's (four uint32 rows per group up to 32 qubits, two uint64 rows above)
    ("linear_function", 9, DEFAULT, "6x16"), ("linear_function", 32, DEFAULT, "16x16"), ("linear_function", 33, DEFAULT, "34x16"),
    ("linear_function", 64, DEFAULT, "64x16"),
    # PTILE-compact: 12-byte qubit records, 8-byte rotation records, one bookkeeping group
    ("pauli", 3, dict(max_rotations=3), "4x12 8x8 1x16"), ("pauli", 20, dict(max_rotations=5), "20x12 8x8 1x16"),
    ("pauli", 24, dict(max_rotations=5, track_solution=True), "24x12 8x8 1x16"),
    # PTILE: 16-byte records throughout; above 16 rotations three bookkeeping groups
    ("pauli", 25, dict(max_rotations=5), "37x16"), ("pauli", 20, dict(max_rotations=9), "37x16"), ("pauli", 32, dict(max_rotations=30), "67x16"),
]


@pytest.mark.parametrize("kind,n,cfg,want", ROWS)
def test_copy_regions_of_every_layout(kind, n, cfg, want):
    assert copy_plan(kind, n, **cfg) == f"copy_envs_kernel [{want}]"


@pytest.mark.parametrize("kind,n,cfg,want", ROWS[::4])
def test_copy_regions_do_not_depend_on_batch_or_weights(kind, n, cfg, want):
    """The side arrays (solution log, layer records) are separate buffers: the state's regions are the layout's alone."""
    for batch in (1, 63, 64, 65, 1 << 20):
        assert copy_plan(kind, n, batch=batch, weights=LAYERS, **cfg) == f"copy_envs_kernel [{want}]"


def test_copy_plan_reports_the_constructor_limits():
    assert copy_plan("clifford", 33, **PLAIN) == _lib_status("UNSUPPORTED")
    assert copy_plan("pauli", 20, max_rotations=33) == _lib_status("UNSUPPORTED")


def _lib_status(name):
    return {"INVALID": -1, "UNSUPPORTED": -3}[name]


DRIVER = r'''
#include <stdio.h>
#include "qgym_done_list.hpp"

using qg::DoneListState;

struct Beliefs {
    int cur;
    uint32_t epoch0, epoch1;
    bool mask_fresh, alt_zero_known, auto_list, fresh, zero_known, tainted;
    uint64_t session;
    bool operator==(const Beliefs &o) const {
        return cur == o.cur && epoch0 == o.epoch0 && epoch1 == o.epoch1 && mask_fresh == o.mask_fresh && alt_zero_known == o.alt_zero_known &&
               auto_list == o.auto_list && fresh == o.fresh && zero_known == o.zero_known && tainted == o.tainted && session == o.session;
    }
};
namespace qg {
struct DoneListProbe {
    static Beliefs get(const DoneListState &d) {
        return {d.cur_, d.epoch_[0], d.epoch_[1], d.mask_fresh_, d.alt_zero_known_, d.auto_list_, d.fresh_, d.zero_known_, d.tainted_, d.session_};
    }
};
}  // namespace qg
static Beliefs B(const DoneListState &d) { return qg::DoneListProbe::get(d); }

static int checks = 0, failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            printf("FAIL line %d: %s\n", __LINE__, #cond);             \
        }                                                              \
    } while (0)

// the library's call sequences (qgym_api.cpp), host bookkeeping only
static bool step(DoneListState &d, uint64_t session, uint64_t step_index) {  // qg_vec_step on a handle whose single step can leave its finishers
    const bool lists = d.step_enters(session);
    const bool zero = lists ? d.before_append() : d.drop();
    if (lists) d.step_left(true, DoneListState::epoch_for(step_index));
    return zero;
}
static DoneListState::Consume reset_done(DoneListState &d, uint64_t session) { return d.reset_consumes(d.enter(session)); }
static bool set_state(DoneListState &d, uint64_t session) {  // qg_vec_set_state: enter, then drop_done_list
    (void)d.enter(session);
    return d.drop();
}

// every history below ends in some state; from there a copy and a set_state must agree on what they enqueue and what they leave
typedef void (*History)(DoneListState &);
static void h_fresh(DoneListState &) {}
static void h_stepped(DoneListState &d) { (void)step(d, 0, 0); }
static void h_auto(DoneListState &d) { (void)reset_done(d, 0); (void)step(d, 0, 1); }
static void h_consumed(DoneListState &d) { (void)reset_done(d, 0); (void)step(d, 0, 1); (void)reset_done(d, 0); }
static void h_captured(DoneListState &d) { (void)reset_done(d, 5); (void)step(d, 5, 2); }
static void h_captured_then_eager(DoneListState &d) { h_captured(d); (void)step(d, 0, 3); }
static void h_fused(DoneListState &d) { h_auto(d); d.fused_ran(DoneListState::epoch_for(4)); }

int main() {
    const History hs[] = {h_fresh, h_stepped, h_auto, h_consumed, h_captured, h_captured_then_eager, h_fused};
    const uint64_t sessions[] = {0, 5, 9};
    for (History h : hs)
        for (uint64_t s : sessions) {
            DoneListState a, b;
            h(a);
            h(b);
            const bool za = a.copied_into(s), zb = set_state(b, s);
            CHECK(za == zb);
            CHECK(B(a) == B(b));
            // afterwards no list is trusted: the next reset_done compacts the `done` flags (which the copy rewrote) instead of reading a list or a mask
            const DoneListState::Consume c = reset_done(a, s);
            CHECK(c.compact && !c.mask);
            CHECK(!a.fused_may_run(a.enter(s)));
        }
    {   // a step left its finishers: the copy forgets them, and the next step's own finishers are what the reset after it reads
        DoneListState d;
        h_auto(d);
        CHECK(B(d).fresh);
        (void)d.copied_into(0);
        CHECK(!B(d).fresh && !B(d).mask_fresh);
        CHECK(!step(d, 0, 7));  // (that step wrote its bits to a mask: the list's length stayed the zero it was)
        const DoneListState::Consume c = reset_done(d, 0);
        CHECK(!c.compact && c.mask);
    }
    {   // a list left by a step whose mask also holds them: the mask's reader zeroed nothing yet, so the copy's drop needs no memset ...
        DoneListState d;
        h_auto(d);
        CHECK(B(d).mask_fresh && B(d).zero_known);
        CHECK(!d.copied_into(0));
        // ... a list left without a mask needs one
        DoneListState e;
        (void)reset_done(e, 0);
        const bool lists = e.step_enters(0);
        CHECK(lists);
        (void)e.before_append();
        e.step_left(false, 0);
        CHECK(e.copied_into(0));
        CHECK(B(e).zero_known);
    }
    {   // a copy inside a capture taints the handle like every captured call: eager calls trust no list afterwards
        DoneListState d;
        (void)d.copied_into(11);
        CHECK(B(d).tainted && d.captured());
        CHECK(!d.enter(0));
    }
    printf("%s %d checks, %d failed\n", failed ? "FAILED" : "ok", checks, failed);
    return failed ? 1 : 0;
}
'''


def test_copy_transition_leaves_what_set_state_leaves(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    src = tmp_path / "copy_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "copy_driver"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    assert out.stdout.startswith("ok "), out.stdout
