"""When an env.step() launch takes the straight-line form of the one-step TILE kernel (qiskit_gym_amd/csrc/qgym_plan.hpp step1_straight), compiled with
g++ and run on the CPU.  That kernel carries none of the generic kernel's per-launch choices, so a launch it is chosen for wrongly computes wrong results
(int64 actions read as int32, lanes past a ragged batch's end running, a missing rewards_seq log, ...): every condition alone must turn it off, the
headline's configuration must turn it on, and the batch limit is group_lanes_pays's, from the device's own compute-unit count."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "qiskit_gym_amd", "csrc")

DRIVER = r'''
#include <stdint.h>
#include <stdio.h>

#include "qgym_plan.hpp"

using namespace qg;

static int checks = 0, failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            if (failed < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
        }                                                              \
    } while (0)

// the headline: CliffordEnv 16q on the line gateset (170 actions), 65 536 envs, MI355X (256 compute units), int32 actions, env.step()
static bool headline_but(Layout layout = LAYOUT_TILE, uint32_t flags = F_GROUP_LANES, size_t A = 170, uint64_t B = 65536, uint32_t cus = 256,
                         bool seq = false, bool clock = false, bool dense = false) {
    return plan::step1_straight(layout, flags, A, B, cus, seq, clock, dense);
}

int main() {
    CHECK(headline_but());
    CHECK(headline_but(LAYOUT_TILE, 0u));  // (F_GROUP_LANES is an output of the same facts, not an input)
    // ---- every condition alone turns it off
    const Layout others[] = {LAYOUT_TILE64, LAYOUT_LFD, LAYOUT_LF8, LAYOUT_PERM, LAYOUT_PERMB, LAYOUT_PAULI};
    for (Layout l : others) CHECK(!headline_but(l));
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES | F_TRACK));      // FEAT: a solution log
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES | F_LAYERS));     // FEAT: layer metrics
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES | F_DONE_LIST));  // LIST
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 65536, 256, false, false, true));  // DENSE
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES | F_ACT64));      // int64 actions
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES | F_INVERTS));    // (not the one-step kernel at all)
    for (uint64_t B : {1ull, 2ull, 63ull, 65ull, 127ull, 255ull, 257ull, 1000ull, 65535ull, 65537ull, 65536ull + 32ull}) CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, B));
    for (uint64_t B : {64ull, 128ull, 192ull, 256ull, 320ull, 65536ull - 64ull, 65536ull + 64ull}) CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, B));
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 256) && !headline_but(LAYOUT_TILE, F_GROUP_LANES, 257) && !headline_but(LAYOUT_TILE, F_GROUP_LANES, 1000));
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 1) && headline_but(LAYOUT_TILE, F_GROUP_LANES, 0));
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 65536, 256, true));         // rewards_seq or dones_seq
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 65536, 256, false, true));  // a kernel clock attached
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 65536, 0));                 // compute units not known: group_lanes_pays says no
    // ---- group_lanes_pays's batch limit, from the device's compute-unit count: three workgroups of 256 envs per compute unit
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 196608, 256) && !headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 229376, 256));
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 196608 + 64, 256) && !headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 262144, 256));
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 3 * 304 * 256, 304) && !headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 3 * 304 * 256 + 64, 304));
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, 229376, 304));
    for (uint64_t B = 64; B <= 400000; B += 64)
        CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, B, 256) == plan::group_lanes_pays(LAYOUT_TILE, 170, B, 256));
    // ---- the 32-bit lane offsets: the largest is the tile's, 16 B x 8 groups per env; bounded whatever compute-unit count a device reports
    CHECK(headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, plan::STEP1_STRAIGHT_MAX_ENVS, 0xFFFFFFFFu));
    CHECK(!headline_but(LAYOUT_TILE, F_GROUP_LANES, 170, plan::STEP1_STRAIGHT_MAX_ENVS + 64, 0xFFFFFFFFu));
    static_assert(plan::STEP1_STRAIGHT_MAX_ENVS * 16ull * 8ull <= (1ull << 32), "a lane's tile offset fits 32 bits");
    static_assert(plan::STEP1_STRAIGHT_MAX_ENVS % 64 == 0, "whole waves");
    printf("%s %d checks, %d failed\n", failed ? "FAILED" : "ok", checks, failed);
    return failed ? 1 : 0;
}
'''


def _hip_include():
    """qgym_plan.hpp includes the shared host/device header, which includes the HIP runtime's (host declarations only are used here)."""
    for root in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    return None


def test_step1_straight_on_the_cpu(tmp_path):
    cxx, inc = shutil.which("g++"), _hip_include()
    if not cxx or not inc:
        pytest.skip("no g++ or no HIP headers")
    src = tmp_path / "step1_straight_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "step1_straight_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    assert out.stdout.startswith("ok "), out.stdout
