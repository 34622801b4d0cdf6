"""The learning signal of the closed loop, pinned after it was measured (profiles/closed_loop.txt): tools/closed_loop.py's
deterministic setting at 256 envs, 30 iterations of OnPolicyRunner.learn for PPO on SurrogateLeggedEnv.  Measured: the mean step
reward over iterations 1-5 is -0.001459, over iterations 26-30 +0.002403, difference +0.003861; the margin asked for is half of
that difference.  Neither the surrogate nor the reward scales were tuned for it."""
import importlib.util
import os
import statistics

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_DIFFERENCE = 0.003861


def test_mean_reward_rises_over_thirty_iterations():
    spec = importlib.util.spec_from_file_location("closed_loop", os.path.join(ROOT, "deep-tracking-control_amd", "tools", "closed_loop.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = tool.learning_curve(256, 30, {})
    first, last = statistics.mean(r[0] for r in rows[:5]), statistics.mean(r[0] for r in rows[25:30])
    print(f"iterations 1-5: {first:+.6f}  iterations 26-30: {last:+.6f}  difference: {last - first:+.6f}")
    assert last - first >= 0.5 * MEASURED_DIFFERENCE
