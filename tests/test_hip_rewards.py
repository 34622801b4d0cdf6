"""GPU: dtc_env_rewards (csrc/rewards.hip) through dtc_amd.rewards against the float64 oracle (tests/golden/reward_oracle.py) on
dtc_amd.synthetic.reward_state inputs, and rewards.patch_env against the reference-captured tests/golden/rewards.npz.

Every continuous term, rew_buf, feet_air_time and pitch_est are held PER TERM to the measure of tests/reward_cases.py,

    max_i |got_i - ref_i| / max(|ref_i|, 1e-2 * max_j |ref_j|)  <=  max(2^-20, 8 * e32),

e32 being the same measure of the oracle's own fp32 run on the same inputs (tests/test_reward_oracle.py asserts 8 * e32 <= 5e-4 for
every case here, and that this measure sees a term scaled by 1 + 2e-3 or short of one dof, which max(1, |ref|) <= 4e-6 did not).
Discrete terms are compared as counts, exactly; last_contacts and the stumble history exactly; state that no active term owns must
come back bit-unchanged.  Against the fixture the bound is the same, but 29.8 * e32 for orientation, orientation_roll and pitch_est
(test_reward_oracle._plane_fit_factor: the reference's fp32 inverse of the plane fit's normal matrix, from the grid alone).  The
episode sums and rew_buf are also held to the kernel's own arithmetic, bit for bit: sums_after == fp32(sums_before + per_term) and
rew_buf == the fp32 sum of the per_term rows in the order of RewardConfig.names, clipped, plus termination (NaN rows: NaN in the
same places; NaN payloads are not compared).  The measure these tests had before,
max |got - ref| / max(1, |ref|) <= 4e-6, stays asserted next to the new one for every quantity: at rows above 1 (rew_buf,
feet_contact_forces and foot_acc in the `all` config) it is the tighter of the two.

One run on an MI355X, the worst case of each column (by error / bound); every entry is error / e32 / bound in units of 1e-7, e32 the
figure of the CPU that ran next to it.  Columns: lite3 / x30 / all = test_every_term_matches_oracle over N = 1, 64, 1024, 4099 and both
clips; alone = test_each_term_alone; sets = test_terms_that_share_state; d<dofs>-b<bodies>-c<commands>-<grid> = test_other_shapes over
N = 5, 67; 20 steps = test_twenty_steps_with_resets; fixture = test_patch_env_matches_reference_fixture.  No case needed a kernel fix;
against the oracle no term needed a multiple of e32 other than 8.  The episode sums per term of the 20-step and fixture runs stay
inside the same rule; the closest is sums:power at 2.7/1.4/10.8.

error / e32 / bound (1e-7)                     lite3                     x30                     all                   alone                    sets            d1-b5-c3-2x2
action_rate                             1.3/1.5/12.3            1.3/1.5/12.3             1.1/1.1/9.5            1.4/1.4/11.3                       -            1.7/1.7/13.5
ang_vel_xy                              1.3/1.3/10.5            1.4/1.4/11.1            1.3/1.3/10.4             1.0/1.0/9.5                       -            1.3/1.3/10.2
base_height                             3.9/3.9/31.4            2.1/2.1/16.4            4.4/4.4/34.9         18.6/18.6/148.6                       -            4.2/4.2/33.3
dof_acc                                 1.3/1.4/11.2            2.2/2.5/19.7            2.2/2.5/19.7            1.8/1.9/15.3                       -            2.0/2.0/16.1
dof_pos_limits                           1.0/1.0/9.5             1.0/1.0/9.5             1.0/1.0/9.5             0.7/0.5/9.5                       -             0.3/0.3/9.5
feet_air_time                           6.7/6.7/53.4            6.7/6.7/53.4            6.7/6.7/53.4            9.9/9.9/78.9            9.9/9.9/78.9          11.0/11.0/88.1
feet_slip                               2.0/1.3/10.3                       -            2.3/1.7/13.3            1.4/1.4/11.2            2.0/1.4/11.2             2.0/1.1/9.5
foot_acc                                2.5/2.5/19.9                       -            2.0/2.0/15.6            2.1/2.1/16.6                       -            4.2/4.2/33.5
hip_pos                                 1.4/1.5/12.3                       -             1.1/1.1/9.5            0.9/1.3/10.5                       -             0.0/0.0/9.5
lin_vel_z                                1.0/1.0/9.5             1.0/1.0/9.5             1.1/1.1/9.5             0.8/0.8/9.5                       -             0.7/0.7/9.5
orientation                              5.3/1.2/9.9             5.3/1.2/9.9             5.3/1.0/9.5            5.0/5.0/40.3            5.0/5.0/40.3             2.4/0.8/9.5
pos_acc                                 1.4/1.3/10.5            1.4/1.3/10.5             1.3/1.2/9.7             1.8/1.1/9.5                       -             1.4/1.1/9.5
power                                   1.7/1.9/15.0                       -            1.7/1.9/15.0            1.7/1.7/13.2                       -             0.8/0.8/9.5
powerchange                             2.4/2.4/19.0            2.4/2.4/19.0            4.1/4.1/32.5            3.5/3.3/26.4                       -            2.5/2.5/19.8
smooth                                  2.2/2.3/18.1                       -            2.1/2.5/19.7            1.7/1.8/14.7                       -            2.6/2.6/21.1
soft_tracking_ang_vel                    0.4/0.9/9.5                       -             0.2/0.7/9.5             0.8/1.1/9.5                       -             0.2/0.7/9.5
soft_tracking_lin_vel                   5.6/4.3/34.6                       -            5.6/4.3/34.6            3.0/3.0/23.7                       -            1.8/1.8/14.2
stand_still                              1.2/1.2/9.8                       -            1.3/1.3/10.3            0.9/1.4/11.2                       -             0.6/0.6/9.5
torques                                 1.4/1.4/11.5                       -            1.6/2.1/16.9            1.3/1.5/12.4                       -             0.6/0.6/9.5
tracking_optimal_footholds           51.4/51.4/411.2         51.7/51.7/413.8         51.4/51.4/411.2       109.7/109.7/878.0                       -            3.8/4.1/32.8
rew                                     2.9/2.9/22.8            1.9/1.9/15.6           24.8/8.5/68.3             1.8/1.1/9.5            2.2/1.8/14.4         48.5/22.3/178.7
feet_air_time (state)                    0.6/0.6/9.5             0.6/0.6/9.5             0.6/0.6/9.5             0.4/0.4/9.5             0.4/0.4/9.5             0.5/0.5/9.5
pitch_est                               3.5/4.0/31.7            3.5/4.0/31.7            2.9/3.8/30.3            2.6/3.9/31.2            2.4/3.4/27.1            1.9/1.7/13.9
dof_vel                                            -             1.3/1.2/9.7            1.3/1.4/11.4            1.7/2.5/19.6                       -             1.0/1.0/9.5
feet_contact_forces                                -            2.1/2.1/16.8            2.0/2.0/15.8            3.0/3.0/23.7                       -            6.6/6.6/53.1
tracking_ang_vel                                   -             0.9/1.2/9.8            1.0/1.5/12.2            0.7/1.3/10.6                       -             0.6/1.2/9.5
tracking_lin_vel                                   -             1.6/0.7/9.5            8.5/7.8/62.7            5.3/5.3/42.0                       -            1.9/1.9/14.9
dof_vel_limits                                     -                       -             1.0/1.0/9.5             0.8/0.8/9.5                       -             0.3/0.3/9.5
orientation_roll                                   -                       -         37.2/14.0/112.0         25.7/55.6/444.8         38.7/38.7/309.4            1.6/1.6/12.8
torque_limits                                      -                       -            1.4/1.4/11.1             0.7/0.7/9.5                       -             0.5/0.5/9.5

error / e32 / bound (1e-7)             d1-b5-c5-11x7         d13-b40-c3-13x5        d64-b40-c5-33x21          d64-b5-c3-11x7          d13-b5-c5-13x5         d12-b17-c4-11x7
action_rate                             1.3/1.3/10.3            1.3/1.4/11.5            1.2/1.4/11.3             1.6/1.1/9.5            1.7/1.7/13.7             1.2/1.2/9.7
ang_vel_xy                               1.0/1.0/9.5             0.9/0.9/9.5             1.1/1.1/9.5             0.8/0.8/9.5             1.1/1.1/9.5             1.2/1.2/9.5
base_height                          22.3/22.3/178.2          10.4/10.4/83.2            8.6/8.6/68.7            4.6/4.6/36.8         16.4/16.4/130.9         15.6/15.6/124.6
dof_acc                                 1.9/1.9/15.6            1.3/2.1/17.0            1.2/1.9/14.8            1.3/1.4/11.3            1.5/1.8/14.6            1.2/1.7/13.2
dof_pos_limits                           0.4/0.4/9.5             0.5/0.5/9.5             1.1/0.4/9.5             0.9/0.9/9.5             0.9/0.9/9.5             0.7/0.7/9.5
feet_air_time                           1.5/1.5/12.4            7.8/7.8/62.2         12.6/12.6/100.9         18.2/18.2/145.5            2.5/2.5/19.8            1.3/1.3/10.3
feet_slip                                1.9/1.1/9.5             1.6/1.0/9.5             1.9/1.0/9.5            1.7/1.4/11.2             1.3/1.1/9.5            1.6/1.4/11.0
foot_acc                                 1.3/0.5/9.5            4.3/4.3/34.4            1.4/1.4/11.1            2.3/2.3/18.4            2.0/2.0/16.3            2.3/2.3/18.3
hip_pos                                  0.7/0.7/9.5             0.8/0.8/9.5            1.5/1.5/11.9             1.1/1.1/9.5             1.2/1.2/9.5            1.1/1.4/10.9
lin_vel_z                                0.6/0.6/9.5             0.8/0.8/9.5             0.7/0.7/9.5             0.9/0.9/9.5             0.8/0.8/9.5             0.9/0.9/9.5
orientation                             3.4/3.4/27.2            8.6/6.2/49.7            4.6/3.3/26.2           15.0/9.5/76.3            2.0/2.0/16.2            5.5/5.5/44.3
pos_acc                                  1.3/1.1/9.5            1.2/1.2/10.0            1.3/1.3/10.0            1.2/1.2/10.0             1.5/1.2/9.5             1.3/1.2/9.5
power                                    0.7/0.7/9.5             1.2/1.2/9.9             1.1/1.1/9.5            1.3/1.4/11.4            1.3/1.3/10.6            1.2/1.4/11.0
powerchange                             2.3/2.3/18.6            1.6/1.6/13.1            2.2/2.2/17.9            2.2/2.2/17.4            2.5/2.5/20.2            1.7/1.7/13.6
smooth                                  2.9/2.9/23.1             1.4/0.9/9.5             1.4/1.1/9.5            1.1/1.2/10.0             1.0/1.0/9.5             1.1/1.1/9.5
soft_tracking_ang_vel                    0.2/0.7/9.5             0.2/0.6/9.5             0.2/0.7/9.5             0.2/0.7/9.5             0.2/0.2/9.5             0.2/0.2/9.5
soft_tracking_lin_vel                   2.6/2.6/20.4            1.3/1.3/10.6            3.6/3.6/29.1            3.8/3.8/30.3            3.2/3.2/26.0            3.6/4.8/38.3
stand_still                              0.4/0.4/9.5             0.9/0.9/9.5             0.4/1.1/9.5             1.0/0.8/9.5            0.8/1.5/12.0             0.7/0.8/9.5
torques                                  0.8/0.8/9.5            2.0/2.2/17.7             1.1/1.1/9.5             1.1/1.2/9.6             0.9/0.6/9.5             1.2/0.6/9.5
tracking_optimal_footholds        158.7/160.3/1282.1            5.4/5.4/43.5            4.9/4.3/34.0      186.6/178.5/1427.9      286.4/226.7/1813.8      182.2/178.0/1424.2
rew                                     2.7/2.7/21.5            2.7/3.3/26.4             0.0/0.0/9.5             0.0/0.0/9.5            9.4/9.4/74.9         65.2/65.2/521.5
feet_air_time (state)                    0.5/0.5/9.5             0.5/0.5/9.5             0.5/0.5/9.5             0.4/0.4/9.5             0.5/0.5/9.5             0.4/0.4/9.5
pitch_est                               2.3/2.3/18.2            2.1/2.1/17.0            1.8/1.8/14.0            1.4/1.4/10.8             3.6/1.0/9.5            3.2/3.8/30.8
dof_vel                                  0.8/0.8/9.5            1.2/1.4/10.9            1.3/1.3/10.1             1.5/1.1/9.5            1.5/1.3/10.5            1.4/1.3/10.7
feet_contact_forces                     4.2/4.2/33.2            5.4/5.4/43.6            1.5/1.5/12.1            2.8/2.8/22.5            2.3/2.3/18.3            9.7/9.7/78.0
tracking_ang_vel                         0.7/1.0/9.5             0.6/1.2/9.8             0.7/1.2/9.7             0.5/1.2/9.7             0.8/1.1/9.5             0.8/1.0/9.5
tracking_lin_vel                        3.4/2.5/20.4            5.1/5.1/40.6             1.1/0.9/9.5            3.4/3.4/27.2            8.8/7.7/61.4            2.9/1.7/13.8
dof_vel_limits                           0.5/0.5/9.5             0.5/0.5/9.5             1.0/0.5/9.5             1.0/1.1/9.5             0.9/0.9/9.5             0.4/0.4/9.5
orientation_roll                     25.5/31.9/255.5             3.5/1.1/9.5            3.9/2.9/23.2         13.3/16.8/134.5             2.0/0.5/9.5         85.5/51.5/411.7
torque_limits                            0.4/0.4/9.5             1.0/1.0/9.5             1.3/1.0/9.5            1.2/1.4/11.4             1.2/0.6/9.5             1.0/1.0/9.5

error / e32 / bound (1e-7)            20 steps lite3            20 steps all           fixture lite3             fixture x30             fixture all
action_rate                             2.4/2.3/18.7            2.0/2.0/15.9            2.6/2.0/15.7            2.2/2.0/16.2            2.1/2.1/16.4
ang_vel_xy                              1.3/1.3/10.4            1.3/1.3/10.6            0.0/1.3/10.4            0.0/1.3/10.0            0.0/1.3/10.0
base_height                          24.0/22.1/176.9         24.1/21.8/174.5         34.1/24.5/196.1            3.3/2.2/17.9         29.8/28.0/224.0
dof_acc                                 2.3/2.3/18.5            2.1/2.1/16.7            2.1/2.2/17.4            2.6/2.3/18.1            2.5/2.5/19.7
dof_pos_limits                           1.0/1.0/9.5             1.1/0.7/9.5             0.0/0.9/9.5             0.0/1.2/9.5             0.8/0.6/9.5
feet_air_time                        18.0/18.0/144.3         18.0/18.0/144.3          0.8/17.8/142.6            1.0/9.7/77.6          0.0/18.4/146.9
feet_slip                               2.2/1.3/10.3            2.2/1.3/10.7            2.2/1.4/11.6                       -            2.0/1.4/10.8
foot_acc                                5.4/5.4/43.0            5.2/5.2/41.4            2.9/3.9/31.2                       -            2.4/2.9/23.2
hip_pos                                 1.8/1.4/11.4            1.7/1.6/12.9            1.4/1.5/11.9                       -            2.0/1.7/13.7
lin_vel_z                                1.0/1.0/9.5             1.1/1.1/9.5             0.0/0.9/9.5             0.0/1.0/9.5             0.0/1.0/9.5
orientation                            12.0/6.9/55.5           11.2/6.9/55.5          47.3/7.5/223.0          46.9/8.4/251.7          73.4/7.5/224.3
pos_acc                                 2.1/1.6/12.5            2.3/1.5/12.0            2.3/1.4/11.6            1.8/1.4/11.4            2.3/1.5/12.3
power                                   1.5/1.5/12.0            1.5/1.5/12.0            2.1/1.7/13.4                       -            2.3/1.6/13.0
powerchange                             4.4/3.9/30.8            5.1/4.8/38.6            3.9/4.1/32.5            4.2/4.3/34.6            3.6/3.9/30.9
smooth                                  2.0/2.0/16.1            2.1/2.1/17.0            2.1/2.2/17.6                       -            2.2/2.2/17.6
soft_tracking_ang_vel                    0.4/0.9/9.5             0.2/0.7/9.5             0.9/0.9/9.5                       -             0.8/0.7/9.5
soft_tracking_lin_vel                   6.3/5.6/45.1            6.3/5.6/45.1            2.0/3.4/27.2                       -            1.4/3.0/24.4
stand_still                             1.4/1.5/12.1            1.7/1.7/13.7            1.5/1.4/11.6                       -            2.2/1.5/12.2
torques                                 2.1/1.8/14.6            2.0/2.1/16.9            2.3/1.8/14.7                       -            2.5/2.0/16.3
tracking_optimal_footholds        274.4/232.6/1860.9      274.4/232.6/1860.9       19.9/176.9/1415.1       52.7/343.2/2745.6      148.8/203.0/1624.3
rew                                     4.3/3.7/29.4        101.8/69.1/552.5            3.3/3.7/29.3            2.7/2.8/22.6         99.0/57.5/459.7
feet_air_time (state)                   1.3/1.3/10.7            1.3/1.3/10.7             0.0/0.6/9.5             0.0/0.6/9.5             0.0/0.6/9.5
pitch_est                              16.5/3.9/31.4            3.0/2.8/22.1           18.5/3.3/97.4           23.4/2.8/84.3           19.6/2.8/83.6
dof_vel                                            -            1.7/1.7/13.6                       -            2.2/1.9/15.4            2.6/1.9/15.4
feet_contact_forces                                -            8.1/8.1/65.1                       -            5.2/7.5/59.6           17.8/9.4/74.9
tracking_ang_vel                                   -            1.3/1.4/10.8                       -            1.1/1.6/12.7            0.8/1.4/10.9
tracking_lin_vel                                   -            6.3/6.1/48.6                       -            1.0/5.6/45.0            1.5/6.6/53.2
dof_vel_limits                                     -             1.2/1.2/9.5                       -                       -             0.0/0.9/9.5
orientation_roll                                   -         56.2/38.2/305.6                       -                       -       148.4/55.0/1638.6
torque_limits                                      -            1.4/1.3/10.4                       -                       -             1.2/1.0/9.5
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import reward_cases as K  # noqa: E402
import reward_oracle as O  # noqa: E402
from dtc_amd import rewards as R  # noqa: E402
from dtc_amd import synthetic as S  # noqa: E402
from test_reward_oracle import TAGS, cfg_from_fixture, fixture_bound, oracle_cfg, run_oracle_sequence, sequence_e32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
INPUTS = set(R._shapes(1, 1, 1, 1, 1))
F32 = np.float32


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rewards")


# worst (error, e32, bound) per (column of the docstring's table, quantity), printed when the module is done
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    cols = list(dict.fromkeys(c for c, _ in RECORD))
    rows = list(dict.fromkeys(k for _, k in RECORD))
    for lo in range(0, len(cols), 6):
        part = cols[lo:lo + 6]
        print("\n" + f"{'error / e32 / bound (1e-7)':28s}" + "".join(f"{c:>24s}" for c in part))
        for k in rows:
            cells = [RECORD.get((c, k)) for c in part]
            if any(cells):
                print(f"{k:28s}" + "".join(f"{'-':>24s}" if v is None else f"{'%.1f/%.1f/%.1f' % tuple(x * 1e7 for x in v):>24s}"
                                           for v in cells))


class _Hold:
    """Collects the per-term comparisons of one case; `done` asserts them all at once, so that a failure shows every figure."""

    def __init__(self, column, label):
        self.column, self.label, self.over, self.lines = column, label, {}, []

    def __call__(self, key, got, ref, e32, b=None):
        err = K.term_err(got, ref)
        b = K.bound(e32) if b is None else b
        assert b <= K.CAP, (self.label, key, e32)
        old = RECORD.get((self.column, key))
        if old is None or not err / b <= old[0] / old[2]:
            RECORD[self.column, key] = (err, e32, b)
        self.lines.append(f"{key}={err:.1e}/{e32:.1e}/{b:.1e}")
        if not err <= b:
            self.over[key] = (err, e32, b)
        if not K.old_err(got, ref) <= K.OLD_BOUND:
            self.over[key + " / max(1, |ref|)"] = (K.old_err(got, ref), K.OLD_BOUND)

    def done(self):
        assert not self.over, (self.label, self.over)


def _rewards(rc, N, layout=K.LITE3, grid=None):
    return R.EnvRewards(N, DEV, rc, grid, feet_indices=layout.feet, penalised_contact_indices=layout.penalised, hip_indices=layout.hips,
                        num_dof=layout.num_dof)


def _load_state(E, env):
    E.feet_air_time.copy_(torch.from_numpy(env["feet_air_time"]))
    E.stumble.copy_(torch.from_numpy(env["stumble"]))
    E.pitch_est.copy_(torch.from_numpy(env["pitch_est"]))


def _call(E, env, **kw):
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in env.items() if k in INPUTS}
    lc = torch.from_numpy(env["last_contacts"].copy()).to(DEV)
    rew, per = E(last_contacts=lc, per_term=True, **inp, **kw)
    return rew.cpu().numpy(), per.cpu().numpy(), lc.cpu().numpy()


def _count(per_term, scale, tol=1e-5):
    """A discrete term's count from term * scale (fp32 products: the count is the nearest integer); tol=1e-3 for an episode sum of
    such products, whose fp32 additions each round at the size of the sum."""
    c = np.asarray(per_term, dtype=np.float64) / scale
    assert np.all(np.isnan(c) | (np.abs(c - np.round(c)) < tol))
    return np.round(c)


def _same_bits(got, want, what):
    """fp32 arrays equal bit for bit (so -0.0 != 0.0), NaN in the same places."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


def _check_identities(rc, per, rew, sums0, sums1, what):
    """The kernel's own arithmetic (r = v * scale; sums = sums + r; rew = rew + r, -ffp-contract=off), restated in numpy fp32."""
    per = per.astype(F32)
    with np.errstate(invalid="ignore"):
        _same_bits(sums1, sums0.astype(F32) + per, f"{what}: episode sums")
        acc = np.zeros(per.shape[1], dtype=F32)
        for i, n in enumerate(rc.names):
            if n != "termination":
                acc = acc + per[i]
        if rc.only_positive_rewards:
            acc = np.where(acc < 0, F32(0), acc)
        if "termination" in rc.scales:
            acc = acc + per[rc.names.index("termination")]
    _same_bits(rew, acc, f"{what}: rew_buf")


def _check_terms(rc, per, ref_per, e32, hold, what):
    for i, n in enumerate(rc.names):
        if n in O.DISCRETE:
            np.testing.assert_array_equal(_count(per[i], rc.scales[n]), _count(ref_per[n], rc.scales[n]), err_msg=f"{what} {n}")
        else:
            hold(n, per[i], ref_per[n], e32[n])


def _check_state(rc, E, lc, env, st, e32, hold, what):
    """The carried state against the oracle's; what no active term owns must be the input, bit for bit."""
    owned = {k for n in rc.names for k in K.OWNS.get(n, ())}
    got = dict(feet_air_time=E.feet_air_time.cpu().numpy(), last_contacts=lc.astype(bool), stumble=E.stumble.cpu().numpy(),
               pitch_est=E.pitch_est.cpu().numpy())
    for k in O.STATE:
        if k not in owned:
            np.testing.assert_array_equal(got[k].view(np.uint8), env[k].view(np.uint8), err_msg=f"{what}: {k} changed")
    np.testing.assert_array_equal(got["last_contacts"], st["last_contacts"], err_msg=what)
    np.testing.assert_array_equal(got["stumble"], st["stumble"], err_msg=what)
    if "feet_air_time" in owned:
        hold("feet_air_time (state)", got["feet_air_time"], st["feet_air_time"], e32["air"])
    if "pitch_est" in owned:
        hold("pitch_est", got["pitch_est"], st["pitch_est"], e32["pitch"])


def _one_launch(column, label, rc, layout, env, sums0, grid_argument=False):
    """One launch of a case of reward_cases against the oracle: terms, rew, state, and the two identities.  `grid_argument`: the
    height grid of `rc` reaches EnvRewards as grid= next to a config that holds the 693-point grid."""
    N = len(sums0[0])
    if grid_argument:
        from dtc_amd.foothold import GridConfig
        E = _rewards(dataclasses.replace(rc, points_x=tuple(S.MEASURED_POINTS_X), points_y=tuple(S.MEASURED_POINTS_Y)), N, layout,
                     GridConfig(points_x=rc.points_x, points_y=rc.points_y))
    else:
        E = _rewards(rc, N, layout)
    assert E.P == env["measured_heights"].shape[1]
    _load_state(E, env)
    E.episode_sums.copy_(torch.from_numpy(sums0))
    rew, per, lc = _call(E, env)
    r64, e32 = K.reference(env, oracle_cfg(rc, layout), sums0)
    hold = _Hold(column, label)
    _check_terms(rc, per, r64["per"], e32, hold, label)
    hold("rew", rew, r64["rew"], e32["rew"])
    _check_state(rc, E, lc, env, r64["st"], e32, hold, label)
    sums1 = E.episode_sums.cpu().numpy()
    _check_identities(rc, per, rew, sums0, sums1, label)
    for i, n in enumerate(rc.names):                        # next to the identity: the sums against the oracle's, as before
        assert K.old_err(sums1[i], r64["sums"][n]) <= K.OLD_BOUND, (label, "sums", n)
    print(f"\n{label} error/e32/bound: " + " ".join(hold.lines))
    hold.done()


@pytest.mark.parametrize("only_positive", [False, True])
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N", K.EVERY_TERM_N)
def test_every_term_matches_oracle(fx, tag, N, only_positive):
    _one_launch(tag, f"{tag} N={N} only_positive={only_positive}", *K.every_term_case(fx, tag, N, only_positive))


@pytest.mark.parametrize("name, termination", K.ALONE_CASES, ids=[n + ("+termination" if t else "") for n, t in K.ALONE_CASES])
def test_each_term_alone(name, termination):
    """Each of the 34 terms as the only active one: no term leans on a neighbour's loads or side effects."""
    _one_launch("alone", f"alone {name}{' +termination' if termination else ''}", *K.alone_case(name, termination))


@pytest.mark.parametrize("names", K.SETS, ids=["+".join(s) for s in K.SETS])
def test_terms_that_share_state(names):
    """feet_slip sees the last_contacts feet_air_time left (or the caller's, alone); orientation and orientation_roll each advance
    pitch_est; foot_clearance owns the stumble history next to the two stumble terms."""
    _one_launch("sets", "set " + "+".join(names), *K.set_case(names))


@pytest.mark.parametrize("N", K.SHAPE_N)
@pytest.mark.parametrize("key", list(K.SHAPES))
def test_other_shapes(fx, key, N):
    """num_dof 1 / 12 / 13 / 64, 0 / 1 / 4 / 16 hips, 5 / 40 bodies with the feet out of order, 0 / 1 / 32 penalised bodies, 3 / 5
    command columns and height grids of 4, 65, 77 and 693 points, every term on."""
    column = key.replace("dof", "d").replace("body", "b").replace("cmd", "c").replace("grid", "")
    _one_launch(column, f"{key} N={N}", *K.shaped_case(fx, key, N), grid_argument=key == K.GRID_ARGUMENT)


@pytest.mark.parametrize("start", ["linspace", "zero"])
@pytest.mark.parametrize("only_positive", [False, True])
def test_sums_and_rew_are_the_kernels_own_arithmetic(fx, only_positive, start):
    """The two identities on NaN / inf rows as well: the sums and rew_buf of a bad row are the fp32 sums of ITS per_term row."""
    N = 259
    rc = K.fixture_rc(fx, "all", only_positive)
    env = K.lite3_state(N, 5)
    for k in ("dof_vel", "contact_forces", "measured_heights", "foot_positions", "base_ang_vel", "commands"):
        env[k][37] = np.nan
    env["torques"][64] = np.inf
    env["root_states"][258, 2] = -np.inf
    sums0 = K.linspace_sums(len(rc.names), N) if start == "linspace" else np.zeros((len(rc.names), N), dtype=F32)
    E = _rewards(rc, N)
    _load_state(E, env)
    E.episode_sums.copy_(torch.from_numpy(sums0))
    rew, per, _ = _call(E, env)
    assert np.isnan(rew[37]) and np.isnan(per[:, 37]).any() and not np.isfinite(per[:, 64]).all()
    _check_identities(rc, per, rew, sums0, E.episode_sums.cpu().numpy(), f"only_positive={only_positive} {start}")


@pytest.mark.parametrize("tag", K.TWENTY["tags"])
def test_twenty_steps_with_resets(fx, tag):
    N, steps, seed = K.TWENTY["N"], K.TWENTY["steps"], K.TWENTY["seed"]
    rc = K.fixture_rc(fx, tag)
    cfg = oracle_cfg(rc)
    E = None
    hold = _Hold("20 steps " + tag, f"{tag} 20 steps")
    for t, (a, b) in enumerate(zip(run_oracle_sequence(cfg, N, steps, seed), run_oracle_sequence(cfg, N, steps, seed, F32))):
        r64 = dict(rew=a[0], per=a[1], sums=a[2], st=a[3])
        e32 = K.e32_of(dict(rew=b[0], per=b[1], st=b[3]), r64)
        env = a[3]                                           # the step's inputs; its state items are the oracle's, after the step
        if E is None:
            E = _rewards(rc, N)
            _load_state(E, O.np_state(S.reward_state(N, seed=seed)))
        sums0 = E.episode_sums.cpu().numpy().copy()
        rew, per, lc = _call(E, env)                         # last_contacts: seq_callback already made it this step's contact
        what = f"{tag} step {t}"
        _check_terms(rc, per, r64["per"], e32, hold, what)
        hold("rew", rew, r64["rew"], e32["rew"])
        np.testing.assert_array_equal(lc.astype(bool), env["last_contacts"], err_msg=what)
        np.testing.assert_array_equal(E.stumble.cpu().numpy(), env["stumble"], err_msg=what)
        hold("feet_air_time (state)", E.feet_air_time.cpu().numpy(), env["feet_air_time"], e32["air"])
        hold("pitch_est", E.pitch_est.cpu().numpy(), env["pitch_est"], e32["pitch"])
        sums1 = E.episode_sums.cpu().numpy()
        _check_identities(rc, per, rew, sums0, sums1, what)
        for i, n in enumerate(rc.names):
            if n in O.DISCRETE:
                np.testing.assert_array_equal(_count(sums1[i], rc.scales[n], 1e-3), _count(r64["sums"][n], rc.scales[n]), err_msg=f"{what} {n}")
            else:
                hold("sums:" + n, sums1[i], r64["sums"][n], K.term_err(b[2][n], r64["sums"][n]))
        ids = torch.from_numpy(np.nonzero(env["reset_buf"])[0]).to(DEV)
        E.feet_air_time[ids], E.pitch_est[ids], E.stumble[ids], E.episode_sums[:, ids] = 0, 0, 0, 0
    print(f"\n{tag} 20 steps error/e32/bound (the last step's): " + " ".join(hold.lines[-(3 + 2 * len(rc.names)):]))
    hold.done()


def test_foot_clearance_from_table(fx):
    N = 1024
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "lite3"))
    cfg = oracle_cfg(rc)
    env = O.np_state(S.reward_state(N, seed=77))
    table = S.reward_table()
    # feet at the low edge of the table: index (x + border) / scale < 2 is clipped to 1, and the reference's px - 2 / py - 2
    # (= -1) wraps to the last row / column; non-finite positions clip to index 1 as well
    g = np.random.default_rng(5)
    fp = env["foot_positions"]
    edge = (-20.0 + 0.15 * g.random((192, 4)) - 0.06).astype(np.float32)    # [-20.06, -19.91): indices 0 and 1 after truncation
    fp[:64, :, 0] = edge[:64]
    fp[64:128, :, 1] = edge[64:128]
    fp[128:192, :, 0], fp[128:192, :, 1] = edge[128:192], edge[128:192][:, ::-1]
    fp[192, 0, 0], fp[193, 1, 1], fp[194, 2, 0] = np.nan, np.nan, -np.inf
    clr_ref = O.foot_clearance_from_table(env["foot_positions"], table.numpy(), 20.0, 0.05, 0.005)
    E = _rewards(rc, N)
    _load_state(E, env)
    out = torch.full((N, 4), float("nan"), device=DEV)
    del env["measured_foot_clearance"]
    rew, per, _ = _call(E, env, height_samples=table.to(DEV), foot_clearance_out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), clr_ref)
    assert np.isfinite(clr_ref).all()
    st = {k: env[k].copy() for k in O.STATE}
    env["measured_foot_clearance"] = clr_ref
    i = rc.names.index("foot_clearance")
    ref = O.term("foot_clearance", env, cfg, st) * rc.scales["foot_clearance"]
    np.testing.assert_array_equal(_count(per[i], rc.scales["foot_clearance"]), _count(ref, rc.scales["foot_clearance"]))
    np.testing.assert_array_equal(E.stumble.cpu().numpy(), st["stumble"])


class _MockEnv:
    """The attributes of LeggedRobotDTC that compute_reward / reset_idx touch, on the device."""

    def __init__(self, cfg, env, N):
        self.cfg, self.num_envs, self.device, self.num_dof = cfg, N, DEV, 12
        self.feet_indices = torch.tensor(S.REWARD_FEET, device=DEV)
        self.penalised_contact_indices = torch.tensor(S.REWARD_PENALISED, device=DEV)
        self.hip_indices = torch.tensor(S.REWARD_HIPS, device=DEV)
        self.command_ranges = dict(lin_vel_x=list(cfg.commands.ranges.lin_vel_x), ang_vel_yaw=list(cfg.commands.ranges.ang_vel_yaw))
        self.rew_buf = torch.zeros(N, device=DEV)
        self.load(env)
        self.stumb_buffer = [torch.from_numpy(((env["stumble"] >> (4 - i)) & 1).astype(bool)).to(DEV) for i in range(5)]

    def load(self, env):
        for k, v in env.items():
            t = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
            if k == "default_dof_pos":
                t = t.unsqueeze(0)
            if k in ("feet_air_time", "pitch_est") and hasattr(self, k):
                continue                                   # the kernel's tensors (patched)
            if k != "stumble":
                setattr(self, k, t)

    def reset_idx(self, env_ids):
        for k in ("feet_air_time", "pitch_est"):
            getattr(self, k)[env_ids] = 0
        for b in self.stumb_buffer:
            b[env_ids] = 0
        for v in self.episode_sums.values():
            v[env_ids] = 0


def test_patch_env_matches_reference_fixture(fx, monkeypatch):
    """patch_env's compute_reward on a mock env, step by step against the reference's own (fp32) run: rew, every term (the launch
    is made to hand out per_term), the episode sums per term and the state at the fixture's strides.  The bound is the one the
    oracle is held to against the same fixture (test_reward_oracle.fixture_bound): max(2^-20, 8 * e32), and 29.8 * e32 for the
    plane-fit quantities, whose fit the reference does through an fp32 inverse."""
    N, steps, stride = (int(v) for v in fx["meta"])
    F = list(S.REWARD_FEET)
    seen = {}
    plain = R.EnvRewards.__call__

    def with_per_term(self, **kw):
        rew, seen["per"] = plain(self, per_term=True, **kw)
        return rew
    monkeypatch.setattr(R.EnvRewards, "__call__", with_per_term)
    for tag in TAGS:
        seed = int(fx["seeds"][TAGS.index(tag)])
        cfg = cfg_from_fixture(fx, tag)
        _, e32s = sequence_e32(oracle_cfg(R.RewardConfig.from_cfg(cfg)), N, steps, seed)
        env = O.seq_begin(S.reward_state(N, seed=seed), F)
        m = _MockEnv(cfg, env, N)
        m.episode_sums = {n: torch.zeros(N, device=DEV) for n in R.RewardConfig.from_cfg(cfg).names}
        Rw = R.patch_env(m)
        rc, names = Rw.cfg, Rw.cfg.names
        hold = _Hold("fixture " + tag, f"{tag} fixture")
        for t in range(steps):
            m.load(env)
            sums0 = Rw.episode_sums.cpu().numpy().copy()
            m.compute_reward()
            e32, what = e32s[t], f"{tag} step {t}"
            rew, per, sums1 = m.rew_buf.cpu().numpy(), seen["per"].cpu().numpy(), Rw.episode_sums.cpu().numpy()
            hold("rew", rew, fx[f"{tag}_rew_{t}"], e32["rew"], fixture_bound("rew", e32["rew"]))
            _check_identities(rc, per, rew, sums0, sums1, what)
            for i, n in enumerate(names):
                ref_per, ref_sums, sc = fx[f"{tag}_per_{t}"][i], fx[f"{tag}_sums_{t}"][i], rc.scales[n]
                assert m.episode_sums[n].data_ptr() == Rw.episode_sums[i].data_ptr()
                if n in O.DISCRETE:
                    np.testing.assert_array_equal(_count(per[i][::stride], sc), _count(ref_per, sc), err_msg=f"{what} {n}")
                    np.testing.assert_array_equal(_count(sums1[i][::stride], sc, 1e-3), _count(ref_sums, sc, 1e-3), err_msg=f"{what} sums {n}")
                else:
                    hold(n, per[i][::stride], ref_per, e32[n], fixture_bound(n, e32[n]))
                    hold("sums:" + n, sums1[i][::stride], ref_sums, e32["sums:" + n], fixture_bound("sums:" + n, e32["sums:" + n]))
            lc = m.last_contacts.cpu().numpy()
            np.testing.assert_array_equal(np.packbits(lc), fx[f"{tag}_contacts_{t}"], err_msg=f"{tag} step {t}")
            np.testing.assert_array_equal(Rw.stumble.cpu().numpy(), fx[f"{tag}_stumble_{t}"], err_msg=f"{tag} step {t}")
            hold("feet_air_time (state)", m.feet_air_time.cpu().numpy()[::4], fx[f"{tag}_air_{t}"], e32["air"], fixture_bound("air", e32["air"]))
            hold("pitch_est", m.pitch_est.cpu().numpy()[::2], fx[f"{tag}_pitch_{t}"], e32["pitch"], fixture_bound("pitch", e32["pitch"]))
            # the driver's env follows the kernel's state, as the env would
            env["last_contacts"] = lc.astype(bool)
            env["feet_air_time"], env["pitch_est"] = m.feet_air_time.cpu().numpy(), m.pitch_est.cpu().numpy()
            env["stumble"] = Rw.stumble.cpu().numpy()
            ids = np.nonzero(env["reset_buf"])[0]
            m.reset_idx(torch.from_numpy(ids).to(DEV))
            O.seq_reset(env, {})
            if t + 1 < steps:
                O.seq_next(env, S.reward_state(N, seed=seed + t + 1), F)
        print(f"\n{tag} fixture error/e32/bound (the last step's): " + " ".join(hold.lines[-(3 + 2 * len(names)):]))
        hold.done()


def _run_once(rc, env, N):
    E = _rewards(rc, N)
    _load_state(E, env)
    rew, per, lc = _call(E, env)
    return [rew, per, lc, E.feet_air_time.cpu().numpy(), E.stumble.cpu().numpy(), E.pitch_est.cpu().numpy(), E.episode_sums.cpu().numpy()]


def test_nan_row_stays_in_its_row(fx):
    N, bad = 256, 37
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "all"))
    env = O.np_state(S.reward_state(N, seed=5))
    clean = _run_once(rc, env, N)
    for k in ("dof_vel", "contact_forces", "measured_heights", "foot_positions", "base_ang_vel", "commands"):
        env[k][bad] = np.nan
    dirty = _run_once(rc, env, N)
    keep = np.arange(N) != bad
    for a, b in zip(clean, dirty):
        rows = (lambda x: np.ascontiguousarray(x.T if x.ndim == 2 and x.shape[0] != N else x))   # env axis first
        np.testing.assert_array_equal(rows(a)[keep].view(np.uint8), rows(b)[keep].view(np.uint8))
    assert np.isnan(dirty[0][bad])


def test_two_launches_same_bits(fx):
    N = 4099
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "all"))
    env = O.np_state(S.reward_state(N, seed=8))
    a, b = _run_once(rc, env, N), _run_once(rc, env, N)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


def test_host_side_arguments(fx):
    """grid= changes the plane-fit grid of the instance, not the caller's config; the clearance comes from ONE source."""
    from dtc_amd.foothold import GridConfig
    rc = R.RewardConfig.from_cfg(cfg_from_fixture(fx, "lite3"))
    before = (rc.points_x, rc.points_y)
    E = R.EnvRewards(64, DEV, rc, GridConfig(points_x=tuple(S.MEASURED_POINTS_X[:11]), points_y=tuple(S.MEASURED_POINTS_Y[:7])),
                     feet_indices=S.REWARD_FEET, penalised_contact_indices=S.REWARD_PENALISED, hip_indices=S.REWARD_HIPS)
    assert (rc.points_x, rc.points_y) == before and E.P == 77
    E = _rewards(rc, 64)
    env = O.np_state(S.reward_state(64, seed=2))
    with pytest.raises(ValueError, match="not both"):
        _call(E, env, height_samples=S.reward_table().to(DEV))
