"""Self-play collection feeds a learner: a plain torch update on `BatchedSynthesis.self_play` samples (examples/az_linear_function.py --
cross-entropy against the visit distribution pi, squared error against the return to go z) raises the share of self-play episodes that end
in success on LinearFunctionGym 4q with device-generated targets.  Checks the whole loop's semantics at once: the device-side reset, the
logged observation, the normalised counts, the value target, the compaction.

The thresholds come from three runs of the example on the MI355X (EXPERIMENTS.md section 23), seeds 0, 1, 2:
    seed 0  0.101 0.147 0.212 0.301 0.425 0.586 0.642 0.674 0.731 0.779 0.780 0.812   start 0.153  end 0.790  gain 0.637
    seed 1  0.140 0.195 0.318 0.392 0.578 0.707 0.720 0.796 0.816 0.844 0.841 0.853   start 0.217  end 0.846  gain 0.629
    seed 2  0.107 0.152 0.180 0.269 0.351 0.512 0.598 0.704 0.731 0.740 0.790 0.775   start 0.147  end 0.768  gain 0.621
GAIN is half the smallest gain (mean of the last three iterations minus mean of the first three) seen over the three seeds; the margin is
there for library GEMM choices in the torch update."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

GAIN = 0.3107  # half the smallest gain over seeds 0, 1, 2
WORST_START = 0.2174  # the greatest mean of the first three iterations over the three seeds


def test_az_on_self_play_samples_learns_to_synthesise():
    from az_linear_function import train

    history = train(seed=0, log=lambda *_: None)
    start, end = sum(history[:3]) / 3, sum(history[-3:]) / 3
    print(f"history {[round(x, 4) for x in history]}: start {start:.4f}, end {end:.4f}")
    assert end - start >= GAIN, (start, end, history)
    assert start < WORST_START + GAIN, (start, history)
