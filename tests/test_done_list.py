"""CPU-side checks of the done-list session protocol (qiskit_gym_amd/csrc/qgym_done_list.hpp): a C++ driver compiled against the header
alone (no HIP, no GPU) walks the call sequences of the library's entry points through DoneListState and checks what each transition
returns and leaves behind.  The expected values are the behaviour of the code the header replaced, where every rule was written out at its
call site; the comments cite those lines as `was <file>:<line>` (the commit before DoneListState)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qiskit_gym_amd", "csrc")

DRIVER = r'''
#include <stdio.h>
#include "qgym_done_list.hpp"

using qg::DoneListState;

struct Beliefs {
    int cur;
    uint32_t epoch0, epoch1;
    bool mask_fresh, alt_zero_known, auto_list, fresh, zero_known, tainted;
    uint64_t session;
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

// The call sites, as the library runs them (only the host-side bookkeeping; `session` is the stream's capture id, 0 = eager).
// qg_vec_step / qg_vec_rollout(T = 1) on a handle whose single step can leave its finishers; `mask`: as bits (TILE / TILE64 / PauliEnv).
struct Step { bool lists, zero; };
static Step step(DoneListState &d, uint64_t session, uint64_t step_index, bool mask = true, bool single = true) {
    const bool lists = d.step_enters(session) && single;
    const bool zero = lists ? d.before_append() : d.drop();
    if (lists) d.step_left(mask, DoneListState::epoch_for(step_index));
    return {lists, zero};
}
// qg_vec_reset_done on TILE / TILE64 (do_reset, only_done, with a list)
static DoneListState::Consume reset_done(DoneListState &d, uint64_t session) { return d.reset_consumes(d.enter(session)); }
// qg_vec_mid_head_sample_step without the in-kernel reset: returns whether the length is zeroed first
static bool sample_step(DoneListState &d, uint64_t session) {
    const bool trusted = d.enter(session);
    const bool zero = d.before_append();
    d.appended(trusted);
    return zero;
}

int main() {
    // ---- starting states ------------------------------------------------------------------------------------------------------
    {   // a fresh handle: was qgym_host.hpp:132-141
        DoneListState d;
        const Beliefs b = B(d);
        CHECK(b.cur == 0 && b.epoch0 == 0 && b.epoch1 == 0);
        CHECK(!b.mask_fresh && b.alt_zero_known && !b.auto_list && !b.fresh && b.zero_known && !b.tainted && b.session == 0);
        CHECK(!d.captured());
    }
    {   // a pooled clone against a fresh handle: was qgym_env.cpp:346-349 -- the length is unknown (a fresh handle knows it is zero); the mask
        // rotation and alt_zero_known are the handle's own and were not touched
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        (void)d.enter(77);                        // captured by its previous owner: tainted
        (void)step(d, 77, 1);                     // cur = 0, epoch0 = 2
        d.fused_ran(DoneListState::epoch_for(2)); // cur = 1, epoch1 = 3, alt_zero_known
        d.handed_on();
        const Beliefs b = B(d), f = B(DoneListState());
        CHECK(b.auto_list == f.auto_list && b.fresh == f.fresh && b.mask_fresh == f.mask_fresh && b.tainted == f.tainted && b.session == f.session);
        CHECK(!b.auto_list && !b.fresh && !b.mask_fresh && !b.tainted && b.session == 0);
        CHECK(!b.zero_known && f.zero_known);
        CHECK(b.cur == 1 && b.epoch0 == 2 && b.epoch1 == 3 && b.alt_zero_known);
        CHECK(d.enter(0) && !d.captured());       // eager calls on the clone are trusted again
        // the first appending launch zeroes the length on the clone (was qgym_api.cpp:275: !list_zero_known), not on a fresh handle
        DoneListState fresh;
        CHECK(sample_step(d, 0));
        CHECK(!sample_step(fresh, 0));
        // its first reset_done compacts, like a fresh handle's
        DoneListState c2;
        c2.handed_on();
        CHECK(reset_done(c2, 0).compact);
    }

    // ---- eager use of a fresh handle --------------------------------------------------------------------------------------------
    {
        DoneListState d;
        CHECK(d.enter(0));                        // was qgym_api.cpp:270: eager, never captured
        // single steps leave nothing until qg_vec_reset_done is in use (was qgym_api.cpp:1015 auto_list)
        Step s = step(d, 0, 0);
        CHECK(!s.lists && !s.zero);
        // the first reset_done compacts (was qgym_api.cpp:886-889: nothing left by a step)
        DoneListState::Consume c = reset_done(d, 0);
        CHECK(c.compact && !c.mask);
        CHECK(B(d).auto_list && B(d).zero_known && !B(d).fresh);  // was qgym_api.cpp:891-893
        // afterwards single steps leave lists; the length is known zero (the reset consumed the list): no memset (was qgym_api.cpp:275)
        s = step(d, 0, 5);
        CHECK(s.lists && !s.zero);
        Beliefs b = B(d);                         // was qgym_api.cpp:282, 291-294
        CHECK(b.fresh && b.mask_fresh && b.zero_known && b.cur == 1 && b.epoch1 == 6);
        // a list-leaving step, then reset_done: no compaction, the mask is read (was qgym_api.cpp:886, 900)
        c = reset_done(d, 0);
        CHECK(!c.compact && c.mask);
        b = B(d);
        CHECK(!b.fresh && !b.mask_fresh && b.zero_known && b.auto_list);
        // the loop goes on alternating the masks
        s = step(d, 0, 6);
        CHECK(s.lists && !s.zero && B(d).cur == 0 && B(d).epoch0 == 7);
        c = reset_done(d, 0);
        CHECK(!c.compact && c.mask);
    }
    {   // a step that appends indices without writing a mask (no done_mask buffer): reset_done skips the compaction but reads no mask
        DoneListState d;
        (void)reset_done(d, 0);
        const Step s = step(d, 0, 0, false);
        CHECK(s.lists && !s.zero && B(d).fresh && !B(d).mask_fresh && !B(d).zero_known && B(d).cur == 0);
        const DoneListState::Consume c = reset_done(d, 0);
        CHECK(!c.compact && !c.mask);
    }

    // ---- two steps without reset_done between them ------------------------------------------------------------------------------
    {   // after a mask-writing step: auto_list off (was qgym_api.cpp:1034), the drop zeroes nothing: mask_fresh && list_zero_known (was :305)
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        const Step s = step(d, 0, 1);
        CHECK(!s.lists && !s.zero);
        CHECK(!B(d).auto_list && !B(d).fresh && !B(d).mask_fresh && B(d).zero_known);
        // later single steps leave nothing until the next reset_done (which compacts: the list was dropped)
        CHECK(!step(d, 0, 2).lists);
        CHECK(reset_done(d, 0).compact);
        CHECK(step(d, 0, 3).lists);
    }
    {   // after a step that appended: the drop zeroes the length (was qgym_api.cpp:305)
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0, false);
        const Step s = step(d, 0, 1);
        CHECK(!s.lists && s.zero);
        CHECK(!B(d).fresh && B(d).zero_known);
        CHECK(!d.drop());                         // nothing left to drop
    }
    {   // a rollout of T > 1 steps after a list-leaving step turns auto_list off as well (was qgym_api.cpp:1218, 1221)
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        const Step s = step(d, 0, 1, true, false);
        CHECK(!s.lists && !s.zero && !B(d).auto_list);
    }
    {   // anything else that changes the flags (set_state, reset) drops the list the same way (was qgym_api.cpp:302-311)
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        CHECK(!d.drop());
        CHECK(B(d).auto_list);                    // (a drop leaves auto_list alone)
        CHECK(reset_done(d, 0).compact);
    }

    // ---- captures ---------------------------------------------------------------------------------------------------------------
    {
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);                      // fresh list and mask, cur = 1
        d.fused_ran(DoneListState::epoch_for(1)); // alt_zero_known (cur = 0)
        // entering a capture clears every belief and taints the handle (was qgym_api.cpp:262-270)
        CHECK(d.enter(42));
        Beliefs b = B(d);
        CHECK(!b.fresh && !b.zero_known && !b.mask_fresh && !b.alt_zero_known && b.tainted && b.session == 42);
        CHECK(b.auto_list && b.cur == 0);         // (auto_list and the mask rotation are not beliefs about the session)
        CHECK(d.captured());                      // was qgym_api.cpp:330
        CHECK(d.alt_needs_zero());                // was qgym_api.cpp:1180
        // inside the capture: the first appending launch zeroes the length, the launches after it are believed again
        Step s = step(d, 42, 2);
        CHECK(s.lists && s.zero);
        CHECK(d.fused_may_run(d.enter(42)));
        DoneListState::Consume c = reset_done(d, 42);
        CHECK(!c.compact && c.mask);
        // after the capture, eager calls are untrusted for good: every reset compacts, no step leaves a list
        CHECK(!d.enter(0));
        CHECK(!d.captured());
        b = B(d);
        CHECK(!b.fresh && !b.zero_known && !b.mask_fresh && !b.alt_zero_known && b.tainted && b.session == 0);
        for (int i = 0; i < 3; ++i) {
            s = step(d, 0, 3 + i);
            CHECK(!s.lists && !s.zero);
            c = reset_done(d, 0);
            CHECK(c.compact && !c.mask);
            CHECK(!d.fused_may_run(d.enter(0)));
        }
        // an untrusted sampling + step launch zeroes the length first and leaves a list nobody trusts (was kernels_policy.hip:1781, 1817)
        CHECK(!sample_step(d, 0));                // (the compacting reset above left the length known zero)
        CHECK(!B(d).fresh && !B(d).zero_known);
        CHECK(reset_done(d, 0).compact);
    }
    {   // two different capture ids: each starts knowing nothing
        DoneListState d;
        (void)reset_done(d, 0);
        CHECK(d.enter(7));
        (void)step(d, 7, 0);
        CHECK(B(d).fresh);
        CHECK(d.enter(9));
        CHECK(!B(d).fresh && !B(d).zero_known && B(d).session == 9);
        DoneListState::Consume c = reset_done(d, 9);
        CHECK(c.compact && !c.mask);
        (void)step(d, 9, 1);
        CHECK(d.enter(7));                        // back to the first id: a new session again
        CHECK(!B(d).fresh && !B(d).zero_known);
        c = reset_done(d, 7);
        CHECK(c.compact && !c.mask);
    }

    // ---- qg_vec_reset_done_step as one launch -----------------------------------------------------------------------------------
    {
        DoneListState d;
        CHECK(!d.fused_may_run(d.enter(0)));      // nothing left by a step (was qgym_api.cpp:1122)
        (void)reset_done(d, 0);
        CHECK(!d.fused_may_run(d.enter(0)));
        (void)step(d, 0, 0);                      // cur = 1, epoch1 = 1
        CHECK(d.fused_may_run(d.enter(0)));
        CHECK(!d.fused_may_run(false));
        CHECK(!d.alt_needs_zero());               // a fresh handle's alternate list is zero
        CHECK(d.cur() == 1 && d.epoch() == 1);    // what the launch reads: done_mask[cur], InitArgs::mask_epoch
        d.fused_ran(DoneListState::epoch_for(1)); // the mask index flips, the epoch is recorded (was qgym_api.cpp:1189-1194)
        Beliefs b = B(d);
        CHECK(b.cur == 0 && b.epoch0 == 2 && b.epoch1 == 1 && d.epoch() == 2);
        CHECK(b.fresh && b.mask_fresh && !b.zero_known && b.alt_zero_known);
        CHECK(d.fused_may_run(d.enter(0)) && !d.alt_needs_zero());
        d.fused_ran(DoneListState::epoch_for(2));
        CHECK(d.cur() == 1 && d.epoch() == 3);
        // the two-launch form after it: reset_done reads the mask, the step leaves a list again
        const DoneListState::Consume c = reset_done(d, 0);
        CHECK(!c.compact && c.mask);
        const Step s = step(d, 0, 3);
        CHECK(s.lists && !s.zero);
        // the fused launch may have appended to its list (envs reset and final again): a drop after it zeroes the length (was :305)
        d.fused_ran(DoneListState::epoch_for(4));
        CHECK(d.drop());
        CHECK(!B(d).fresh && !B(d).mask_fresh && B(d).zero_known);
    }
    {   // without auto_list (no reset_done yet on this handle) the one launch does not run
        DoneListState d;
        (void)d.enter(0);
        d.step_left(true, 1);
        CHECK(!d.fused_may_run(true));
    }

    // ---- the sampling + step kernels ------------------------------------------------------------------------------------------
    {   // appending form: zero the length unless known zero, then a trusted list without a mask (was kernels_policy.hip:1778-1781, 1817)
        DoneListState d;
        CHECK(!sample_step(d, 0));
        CHECK(B(d).fresh && !B(d).zero_known && !B(d).mask_fresh);
        DoneListState::Consume c = reset_done(d, 0);
        CHECK(!c.compact && !c.mask);
        CHECK(!sample_step(d, 0));                // the reset consumed the list
        CHECK(sample_step(d, 0));                 // the list of the launch before was never consumed: zeroed first
        CHECK(B(d).fresh);
        // after a mask-writing step the length is known zero, but the step's finishers were never consumed: zeroed all the same
        // (was qgym_api.cpp:275: `|| done_list_fresh`)
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        CHECK(B(d).fresh && B(d).zero_known);
        CHECK(sample_step(d, 0));
    }
    {   // in-kernel reset (small batches): the launch only enters the session (was kernels_policy.hip:1778-1779, 1792), so the beliefs
        // stay what the launch before left.  After a list-leaving qg_vec_step, a qg_vec_reset_done that follows would still trust that
        // step's list: pinned as it is
        DoneListState d;
        (void)reset_done(d, 0);
        (void)step(d, 0, 0);
        const Beliefs before = B(d);
        (void)d.enter(0);
        const Beliefs after = B(d);
        CHECK(after.fresh == before.fresh && after.mask_fresh == before.mask_fresh && after.zero_known == before.zero_known && after.cur == before.cur);
        CHECK(after.fresh && after.mask_fresh);
    }

    // ---- PauliEnv's reset_done --------------------------------------------------------------------------------------------------
    {   // from the mask when the step before left bits in this session (was qgym_api.cpp:865-867)
        DoneListState d;
        CHECK(!d.pauli_reset_consumes(d.enter(0)));  // nothing left by a step: compact
        CHECK(B(d).auto_list);
        // The compacting reset leaves list_zero_known as it was (true here) although compact_done wrote a non-zero length: wrong, but
        // harmless today -- nothing appends to a PauliEnv list (its LIST step writes the mask), so no append trusts that zero.
        CHECK(B(d).zero_known);
        const Step s = step(d, 0, 0);
        CHECK(s.lists && !s.zero);
        CHECK(d.pauli_reset_consumes(d.enter(0)));
        CHECK(!B(d).fresh && !B(d).mask_fresh);
        CHECK(!d.pauli_reset_consumes(d.enter(0)));  // consumed
        // a step that appended without bits, or an untrusted session, compacts
        d.appended(true);
        CHECK(!d.pauli_reset_consumes(true));
        (void)step(d, 0, 1);
        CHECK(!d.pauli_reset_consumes(false));
    }

    // ---- drop on a handle that never appended (LF8 / PERM: no list) enqueues nothing ---------------------------------------------
    {
        DoneListState d;
        for (int i = 0; i < 3; ++i) {
            (void)d.enter(0);
            CHECK(!d.drop());
        }
        (void)d.enter(5);                         // captured
        CHECK(!d.drop());
        (void)d.enter(0);
        CHECK(!d.drop());
        d.handed_on();
        CHECK(!d.drop());
    }

    // ---- the mask epoch of a step index (was qgym_api.cpp:287): never 0, the buffers' initial hint --------------------------------
    CHECK(DoneListState::epoch_for(0) == 1u);
    CHECK(DoneListState::epoch_for(41) == 42u);
    CHECK(DoneListState::epoch_for(0x7FFFFFFFull) == 0x80000000u);
    CHECK(DoneListState::epoch_for(0x80000000ull) == 1u);
    CHECK(DoneListState::epoch_for((1ull << 32) + 5) == 6u);
    CHECK(DoneListState::epoch_for(~0ull) == 0x80000000u);

    printf("%s %d checks, %d failed\n", failed ? "FAILED" : "ok", checks, failed);
    return failed ? 1 : 0;
}
'''


def test_done_list_protocol_on_the_cpu(tmp_path):
    """The header compiles with a plain C++17 compiler (no HIP, no ROCm) and every transition does what the call sites did before it."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    src = tmp_path / "done_list_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "done_list_driver"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    assert out.stdout.startswith("ok "), out.stdout
