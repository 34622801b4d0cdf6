"""TEST INFRASTRUCTURE: inputs of the dtc_sim_balance tests (tests/test_sim_balance_host.py on the CPU, tests/test_hip_sim_balance.py
on the GPU), as numpy arrays in the layout of the env's tensors.  The kernel reads what a surrogate step wrote, whatever that is,
so the states are built directly, one scenario per branch of the rule (SCENARIOS): a base at 0.3 m over feet at the corners of the
default stance (or where the scenario puts them), a stance mask, the base's offset from the stance centre in the body frame, a lean
and its rate, and the step count since the reset.  Env n of round r takes scenario (r N + n) mod len(SCENARIOS) under a seeded yaw,
position and (tilted) roll and pitch, so ceil(len / N) rounds of N envs take every branch whatever N is; random values stand in
every row and column the kernel must leave alone.  tests/test_sim_balance_host.py asserts on the CPU that they do."""
import numpy as np

import sim_balance_oracle as BO

F = np.float32
FEET, B = (4, 8, 12, 16), 17
CORNERS = ((0.17, 0.1), (0.17, -0.1), (-0.17, 0.1), (-0.17, -0.1))                  # FL, FR, HL, HR, body frame
HEIGHT = 0.3


class Balance:
    """The fields of dtc_amd.sim.BalanceConfig at their defaults, for the oracle alone."""
    gravity, h_min, lean_eps, fall_angle, fall_force = 9.81, 0.05, 1e-3, 0.8, 200.0

    def __init__(self, com_offset=(0.0, 0.0)):
        self.com_offset = com_offset


def constants(tilted):
    """balance_dict of the GPU cases: the tilted ones carry a centre of mass 2 cm ahead of the base's origin."""
    return BO.balance_dict(Balance((0.02, 0.0) if tilted else (0.0, 0.0)), 0.005, 4)


def _s(stance, off=(0.0, 0.0), lean=(0.0, 0.0, 0.0, 0.0), ep=7, feet=None, foot_z=(0.0, 0.0, 0.0, 0.0), force=None):
    return dict(stance=stance, off=off, lean=lean, ep=ep, feet=feet or CORNERS, foot_z=foot_z, force=force)


ALL = (1, 1, 1, 1)
SCENARIOS = (
    _s(ALL),                                                                          # upright over four feet
    _s(ALL, lean=(0.2, 0.1, 0.0, 0.0)),                                               # restoring
    _s(ALL, lean=(0.01, 0.0, -1.0, 0.0)),                                             # lands by the sign change
    _s(ALL, lean=(0.005, 0.0, -0.02, 0.0)),                                           # lands under lean_eps
    _s(ALL, off=(0.0, 0.15)),                                                         # outside, nearest to an edge
    _s(ALL, off=(0.25, 0.2), lean=(0.05, 0.02, 0.1, 0.0)),                            # outside, nearest to a vertex
    _s(ALL, lean=(0.1, -0.2, 0.0, 0.1), foot_z=(0.0, 0.04, 0.08, 0.02)),              # the highest foot is not the first
    _s((1, 1, 0, 1), off=(0.05, -0.03), lean=(0.0, 0.15, 0.0, 0.0)),                  # a clockwise triangle, inside
    _s((1, 1, 0, 1), off=(-0.1, 0.08)),                                               # the same triangle, outside its long edge
    _s((1, 1, 0, 1), feet=((0.17, -0.1), (0.17, 0.1), (-0.17, 0.1), (-0.17, 0.1)), off=(0.05, 0.03), lean=(0.1, 0.0, 0.0, 0.0)),   # counter-clockwise
    _s((1, 1, 0, 1), feet=((0.17, -0.1), (0.17, 0.1), (-0.17, 0.1), (-0.17, 0.1)), off=(0.3, 0.0)),                               # ... and outside it
    _s((1, 0, 0, 1), off=(0.03, 0.04)),                                               # the diagonal pair
    _s((1, 0, 1, 0), lean=(0.0, -0.3, 0.0, -0.5)),                                    # two feet of one side
    _s((1, 0, 1, 0), off=(-0.3, 0.1), lean=(0.0, 0.0, 0.2, 0.0)),                     # ... nearest to the segment's end
    _s((0, 1, 0, 0), lean=(0.1, 0.1, 0.0, 0.0)),                                      # one foot
    _s((0, 0, 0, 0), lean=(0.1, 0.0, 0.5, 0.2)),                                      # airborne: the rate is kept
    _s((1, 0, 1, 0), lean=(0.3, 0.2, 1.0, 0.5), ep=1),                                # the step after a reset
    _s((1, 0, 1, 0), lean=(0.0, -0.79, 0.0, -1.0), force=50.0),                       # a fall: the force is raised
    _s((0, 0, 0, 0), lean=(0.9, 0.3, 0.0, 0.0), force=250.0),                         # a fall onto a crash force: kept
    _s(ALL, lean=(0.9, 0.0, 0.0, 0.0), force=0.0),                                    # a fall over four feet (restoring, still beyond)
)


def state(N, tilted, round_=0, nan_rows=()):
    """The tensors dtc_sim_balance reads and writes for the envs of round `round_`."""
    st = dict(root_states=np.zeros((N, 13)), base_pos=np.zeros((N, 3)), base_quat=np.zeros((N, 4)), projected_gravity=np.zeros((N, 3)),
              base_lin_vel=np.zeros((N, 3)), base_ang_vel=np.zeros((N, 3)), rigid_body_state=np.zeros((N, B, 13)),
              contact_forces=np.zeros((N, B, 3)), lean=np.zeros((N, 4)), contact_filt=np.zeros((N, 4), dtype=bool),
              episode_length_buf=np.zeros(N, dtype=np.int64))

    def mul(a, b):
        return np.concatenate([a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3]), [a[3] * b[3] - a[:3] @ b[:3]]])
    for n in range(N):
        i = round_ * N + n
        sc = SCENARIOS[i % len(SCENARIOS)]
        g = np.random.default_rng(500 + i + (10000 if tilted else 0))
        yaw = (2 * g.random() - 1) * np.pi
        c, s = np.cos(yaw), np.sin(yaw)
        centre = np.array([1.0 + 3 * g.random(), 1.0 + 3 * g.random()])
        roll, pitch = (0.6 * g.random(2) - 0.3) if tilted else (0.0, 0.0)
        q = mul(mul(np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.array([0, np.sin(pitch / 2), 0, np.cos(pitch / 2)])),
                np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)]))
        rb, cf = g.standard_normal((B, 13)), 50 * g.standard_normal((B, 3))
        for l in range(4):
            fx, fy = sc["feet"][l]
            rb[FEET[l], 0:3] = centre[0] + c * fx - s * fy, centre[1] + s * fx + c * fy, sc["foot_z"][l]
        ox, oy = sc["off"]
        base = np.array([centre[0] + c * ox - s * oy, centre[1] + s * ox + c * oy, HEIGHT])
        if sc["force"] is not None:
            cf[0] = (0.0, 0.0, sc["force"])
        lp, lv = sc["lean"][:2], sc["lean"][2:]                                        # the scenario's lean is in the body's yaw frame
        st["lean"][n] = c * lp[0] - s * lp[1], s * lp[0] + c * lp[1], c * lv[0] - s * lv[1], s * lv[0] + c * lv[1]
        st["root_states"][n] = np.concatenate([base, q, g.standard_normal(6)])
        st["base_pos"][n], st["base_quat"][n] = base, q
        st["projected_gravity"][n], st["base_lin_vel"][n], st["base_ang_vel"][n] = g.standard_normal(3), g.standard_normal(3), g.standard_normal(3)
        st["rigid_body_state"][n], st["contact_forces"][n] = rb, cf
        st["contact_filt"][n], st["episode_length_buf"][n] = np.array(sc["stance"], dtype=bool), sc["ep"]
    st = {k: (v.astype(F) if v.dtype == np.float64 else v) for k, v in st.items()}
    for n in nan_rows:
        for name, a in st.items():
            if a.dtype == F:
                a[n] = np.nan
    return st


def rounds(N):
    return -(-len(SCENARIOS) // N)


def expected(st, tilted, dtype=F):
    """The oracle's outputs for `st`, and its trace."""
    trace = {}
    return BO.balance(st, FEET, constants(tilted), dtype, trace), trace
