"""The host side of the one-step TILE kernel's group table (qiskit_gym_amd/csrc/qgym_plan.hpp gate_group_bytes), compiled with g++ and run on the CPU:
the packed group bytes a wave holds across its lanes -- byte i = g0 | g1 << 4 of action i, as decoded from the table's action words
(q0 | q1 << 5 | M << 10; a qubit's group is q >> 1 with Z rows, q >> 2 without) -- for 1 to 300 actions.  Beyond 256 the kernel does not use the
table: the first 256 are still packed, and nothing is written past the table's 64 dwords."""
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

static uint64_t rng_state = 0x1234567ull;
static uint32_t rnd() { return (uint32_t)(splitmix64(rng_state++) >> 16); }

int main() {
    // ---- packed group bytes against the groups decoded from the entries
    for (int has_z = 0; has_z < 2; ++has_z)
        for (size_t A = 1; A <= 300; ++A) {
            GateEntry table[300];
            for (size_t i = 0; i < A; ++i) table[i] = GateEntry{rnd() & 0x3FFFFFFu, 0.5f};
            uint32_t out[plan::GROUP_TABLE_DWORDS + 2];
            out[plan::GROUP_TABLE_DWORDS] = out[plan::GROUP_TABLE_DWORDS + 1] = 0xDEADBEEFu;
            plan::gate_group_bytes(&table[0].ops, sizeof(GateEntry) / sizeof(uint32_t), A, has_z, out);
            const uint32_t gsh = has_z ? 1u : 2u;
            for (size_t i = 0; i < 4 * plan::GROUP_TABLE_DWORDS; ++i) {
                const uint32_t byte = (out[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                if (i < A) {
                    const uint32_t q0 = table[i].ops & 31u, q1 = (table[i].ops >> 5) & 31u;
                    CHECK(byte == ((q0 >> gsh) | ((q1 >> gsh) << 4)));
                } else {
                    CHECK(byte == 0);
                }
            }
            CHECK(out[plan::GROUP_TABLE_DWORDS] == 0xDEADBEEFu && out[plan::GROUP_TABLE_DWORDS + 1] == 0xDEADBEEFu);
        }
    // ---- when the kernel uses the table: it holds every action, and the launch is at most three workgroups per compute unit
    CHECK(plan::group_lanes_pays(LAYOUT_TILE, 1, 1, 256) && plan::group_lanes_pays(LAYOUT_TILE, 256, 65536, 256));
    CHECK(!plan::group_lanes_pays(LAYOUT_TILE, 257, 65536, 256));
    CHECK(plan::group_lanes_pays(LAYOUT_TILE, 170, 196608, 256) && !plan::group_lanes_pays(LAYOUT_TILE, 170, 196609, 256));
    CHECK(!plan::group_lanes_pays(LAYOUT_TILE, 170, 262144, 256));
    CHECK(plan::group_lanes_pays(LAYOUT_TILE, 170, 3 * 304 * 256, 304) && !plan::group_lanes_pays(LAYOUT_TILE, 170, 3 * 304 * 256 + 1, 304));
    CHECK(!plan::group_lanes_pays(LAYOUT_TILE, 170, 1, 0));  // compute units not known
    CHECK(!plan::group_lanes_pays(LAYOUT_TILE64, 170, 64, 256) && !plan::group_lanes_pays(LAYOUT_LFD, 170, 64, 256));
    static_assert(plan::GROUP_LANES_MAX_ACTIONS == 4 * plan::GROUP_TABLE_DWORDS && plan::GROUP_TABLE_DWORDS == 64, "one dword per lane of a wave");
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


def test_group_table_on_the_cpu(tmp_path):
    cxx, inc = shutil.which("g++"), _hip_include()
    if not cxx or not inc:
        pytest.skip("no g++ or no HIP headers")
    src = tmp_path / "group_table_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "group_table_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FAIL" not in out.stdout, out.stdout
    assert out.stdout.startswith("ok "), out.stdout
