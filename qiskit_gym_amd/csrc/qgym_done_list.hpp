// qgym_done_list.hpp -- what the host believes about a handle's list of finished envs and its two done masks.  Host-only, no HIP
// (tests/test_done_list.py compiles it on its own).
//
// ---- the list of finished envs (done_list: [B] indices, then {length, reader ticket}) --------------------------------------------
// Device-side facts: a LIST step kernel (and the sampling + step kernels) APPENDS to the list, so the length must be zero when it starts; the reset
// kernel that consumes a list zeroes the length again (list_count_take); compact_done zeroes it itself.  What the host knows about the length is exact
// only for launches it has enqueued eagerly, in order: anything captured into a caller's graph runs later, any number of times, between whatever else
// the caller enqueues.  So the host's belief (fresh_, zero_known_) is scoped to a SESSION -- one stream capture (its capture id), or eager execution
// on a handle none of whose list launches were ever captured:
//   * a new session starts with nothing known: its first appending launch is preceded by a memset of the length (captured with it), its first
//     qg_vec_reset_done compacts the `done` flags itself;
//   * once anything was captured (tainted_), eager calls trust nothing: no LIST instantiations, every reset_done compacts;
//   * inside a session the launches run in the order they were enqueued, so the belief is exact there.
// Appends are clamped to the list's B entries on the device as well (done_list_append), so a misuse cannot write past the allocation.
// The transitions only update the belief and return what the caller must enqueue; the device pointers (done_list, the idle and alternate lists,
// done_mask[2]) and their rotations stay in qg_vec.
#pragma once

#include <stdint.h>

namespace qg {

class DoneListState {
public:
    struct Consume { bool compact, mask; };  // compact_done first (no step left the finishers); read done_mask[cur()] (it left them as bits)
    // the number a mask-writing launch stamps its buffer's hint word with (never 0, the buffers' initial content)
    static uint32_t epoch_for(uint64_t step_index) { return ((uint32_t)step_index & 0x7FFFFFFFu) + 1u; }

    // A handle from the pool (qg_env_clone) carries its previous owner's session state: it starts like a fresh handle, except that the
    // list's length is unknown (always safe: the next appending launch zeroes it first).  The mask rotation and alt_zero_known_ stay.
    void handed_on() { auto_list_ = fresh_ = mask_fresh_ = zero_known_ = tainted_ = false; session_ = 0; }

    // Every call that touches the list or the `done` flags enters its stream's session first (0: eager, else the capture id).
    // Returns whether the beliefs may be acted on: inside a capture, or eagerly on a handle that was never captured.
    bool enter(uint64_t session) {
        if (session != session_) {
            session_ = session;
            fresh_ = zero_known_ = mask_fresh_ = alt_zero_known_ = false;
            if (session) tainted_ = true;
        }
        return session != 0 || !tainted_;
    }
    bool captured() const { return session_ != 0; }  // a launch enqueued now keeps its arguments for every replay
    // qg_vec_step / qg_vec_rollout enter their session: whether a single step may leave its finishers (trusted, reset_done in use)
    bool step_enters(uint64_t session) {
        const bool trusted = enter(session);
        if (fresh_) auto_list_ = false;  // the last list was never consumed: this caller steps without qg_vec_reset_done
        return trusted && auto_list_;
    }
    // before a launch that appends: whether the length must be zeroed first
    bool before_append() {
        const bool zero = !zero_known_ || fresh_;
        fresh_ = mask_fresh_ = false;
        zero_known_ = true;
        return zero;
    }
    void appended(bool trusted) { fresh_ = trusted; zero_known_ = mask_fresh_ = false; }  // an untrusted list is never consumed
    // a list-leaving step ran (trusted: it was allowed to): it appended its finishers, or wrote them to the mask that is not the current one
    void step_left(bool mask, uint32_t epoch) { appended(true); if (mask) wrote_mask(epoch); }
    // A list describes the `done` flags of the step that wrote it only: anything else that changes the flags drops it first.  Whether
    // its length must be zeroed (which only the list's consumer would have done).
    bool drop() {
        const bool zero = fresh_ && !(mask_fresh_ && zero_known_);
        if (fresh_) zero_known_ = true;
        fresh_ = mask_fresh_ = false;
        return zero;
    }
    // qg_vec_copy_envs into this handle: the copied envs' `done` flags are their sources', so the list and the masks describe nothing any
    // more -- what qg_vec_set_state leaves (enter the stream's session, drop).  Whether the list's length must be zeroed.
    bool copied_into(uint64_t session) {
        (void)enter(session);
        return drop();
    }
    // qg_vec_reset_done on TILE / TILE64: its kernel consumes the list and zeroes the length (list_count_take)
    Consume reset_consumes(bool trusted) {
        const bool left_by_step = trusted && fresh_;  // the step before recorded its finishers itself (a list, or bits + a list)
        const Consume c{!left_by_step, left_by_step && mask_fresh_};
        fresh_ = mask_fresh_ = false;
        zero_known_ = auto_list_ = true;
        return c;
    }
    // PauliEnv's qg_vec_reset_done: whether the step before (ptile_step1c_kernel<LIST>) left its finishers as bits.  zero_known_
    // stays as it was, even after a compacting reset: nothing appends to a PauliEnv list.
    bool pauli_reset_consumes(bool trusted) {
        const bool from_mask = trusted && fresh_ && mask_fresh_;
        fresh_ = mask_fresh_ = false;
        auto_list_ = true;
        return from_mask;
    }
    // qg_vec_reset_done_step as one launch: reads done_mask[cur()] and the list, appends to the alternate list, writes the other mask
    bool fused_may_run(bool trusted) const { return trusted && fresh_ && mask_fresh_ && auto_list_; }
    bool alt_needs_zero() const { return !alt_zero_known_; }
    // (after the caller's rotation: the list just appended to is the current one, the idle one the launch zeroed is the alternate)
    void fused_ran(uint32_t epoch) { wrote_mask(epoch); fresh_ = alt_zero_known_ = true; zero_known_ = false; }

    int cur() const { return cur_; }                 // done_mask[cur()]: the mask the last list-leaving launch wrote
    uint32_t epoch() const { return epoch_[cur_]; }  // ... and its epoch (InitArgs::mask_epoch for its reader)

private:
    friend struct DoneListProbe;  // tests/test_done_list.py
    // (and appended nothing: the length is still the zero before_append made sure of)
    void wrote_mask(uint32_t epoch) { cur_ ^= 1; epoch_[cur_] = epoch; mask_fresh_ = zero_known_ = true; }
    int cur_ = 0;
    uint32_t epoch_[2] = {0, 0};  // StepArgs::done_epoch of the launch that wrote each buffer
    bool mask_fresh_ = false;     // done_mask[cur_] (+ the list: envs reset and final again inside the fused launch) holds the final envs
    bool alt_zero_known_ = true;  // done_list_alt's length is known to be zero
    bool auto_list_ = false;      // qg_vec_reset_done is in use on this handle: single steps leave the envs they finish themselves
    bool fresh_ = false;          // the list holds the finished envs (written by the step that ended them)
    bool zero_known_ = true;      // the list's length is known to be zero (creation, a memset, or its consumer ran)
    bool tainted_ = false;        // some launch that touches the list was captured into a caller's graph: eager calls trust nothing
    uint64_t session_ = 0;        // 0 = eager execution, else the stream capture id the beliefs belong to
};

}  // namespace qg
