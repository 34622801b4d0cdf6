"""TEST INFRASTRUCTURE: numpy restatement of dtc_sim_contacts (csrc/sim_contacts.hip; include/dtc_hip.h states the operations C1..C5),
operation by operation: with dtype float32 every value below is one single-rounded float32 operation in the kernel's order, so the
kernel's outputs are compared bit for bit; with dtype float64 the same rule runs in double for the property tests.  Nothing here
imports the package's kernels."""
import numpy as np

import sim_oracle as O

F = np.float32
FLAGS = ("leg_contact", "stumbled")
CONSTANTS = ("body_radius", "stiffness", "max_force", "probe", "stumble_height", "wall_damping", "min_speed")
THIGH_S, SHANK_S = (0.25, 0.5, 0.75), (0.0, 0.25, 0.5, 0.75)


def contact_dict(c):
    """The constants of a dtc_amd.sim.ContactConfig as the kernel receives them (float32 scalars)."""
    return dict({name: F(getattr(c, name)) for name in CONSTANTS}, shanks=tuple(int(v) for v in c.shanks))


def knee_tables(cfg, dtype=F):
    from dtc_amd import sim as SIM
    return {k: np.asarray(v, dtype=dtype) for k, v in SIM.knee_tables(cfg).items()}


def terrain_height(k, hs, x, y, dtype=F):
    """sim_oracle.terrain_height (step 5 of dtc_sim_step) in `dtype`, with the float -> integer conversion spelled out where numpy
    leaves it undefined: a NaN gives index 0, as on the device; then the clamp.  Equal to sim_oracle's on every finite point."""
    T = dtype
    wx = (x + T(k["border_size"])) / T(k["horizontal_scale"])
    wy = (y + T(k["border_size"])) / T(k["horizontal_scale"])
    big = 2.0 ** 62
    cx = np.clip(np.nan_to_num(np.trunc(wx).astype(np.float64), nan=0.0, posinf=big, neginf=-big), -big, big).astype(np.int64)
    cy = np.clip(np.nan_to_num(np.trunc(wy).astype(np.float64), nan=0.0, posinf=big, neginf=-big), -big, big).astype(np.int64)
    cx, cy = np.clip(cx, 0, k["rows"] - 2), np.clip(cy, 0, k["cols"] - 2)
    h = np.minimum(np.minimum(hs[cx, cy], hs[cx + 1, cy]), hs[cx, cy + 1])
    return h.astype(T) * T(k["vertical_scale"])


def knee_world(st, tables, knee, dtype=F):
    """C1: the knee positions [N,4,3] in the world."""
    T = dtype
    N = st["base_pos"].shape[0]
    B, q = st["base_pos"].astype(T), st["base_quat"].astype(T)
    dq = (st["dof_pos"].astype(T) - np.asarray(tables["default_dof_pos"], dtype=T)).reshape(N, 4, 3)
    nom, J = np.asarray(knee["knee_nominal"], dtype=T), np.asarray(knee["knee_jacobian"], dtype=T)
    v = nom[None] + ((J[None, :, :, 0] * dq[:, :, None, 0] + J[None, :, :, 1] * dq[:, :, None, 1]) + J[None, :, :, 2] * dq[:, :, None, 2])
    qx, qy, qz, qw = (q[:, i, None] for i in range(4))
    two = T(2)
    tx, ty, tz = two * (qy * v[..., 2] - qz * v[..., 1]), two * (qz * v[..., 0] - qx * v[..., 2]), two * (qx * v[..., 1] - qy * v[..., 0])
    cx, cy, cz = qy * tz - qz * ty, qz * tx - qx * tz, qx * ty - qy * tx
    rot = np.stack([(v[..., 0] + qw * tx) + cx, (v[..., 1] + qw * ty) + cy, (v[..., 2] + qw * tz) + cz], axis=-1)
    return B[:, None, :] + rot


def contacts(st, k, ck, tables, knee, height_samples, dtype=F, trace=None):
    """dtc_sim_contacts on the state `st` a surrogate step left behind (base_pos, base_quat, dof_pos [N,12] dense, rigid_body_state,
    contact_forces).  `k`: sim_oracle.config_dict (feet, thighs, the table's shape and scales), `ck`: contact_dict, `knee`:
    knee_tables.  Returns dict(contact_forces, rigid_body_state, leg_contact, stumbled): copies with the kernel's rows rewritten;
    `st` is left unchanged.  `trace`, a dict, receives the intermediate values for the property tests."""
    T = dtype
    height = lambda kk, hs, x, y: terrain_height(kk, hs, x, y, T)                  # noqa: E731
    c = {name: T(ck[name]) for name in CONSTANTS}
    N = st["base_pos"].shape[0]
    feet, thighs, shanks = list(k["feet"]), list(k["thighs"]), list(ck["shanks"])
    rb = np.array(st["rigid_body_state"], copy=True)
    cf = np.array(st["contact_forces"], copy=True)
    if T != F:                                                                      # the property tests read the rule's own precision
        rb, cf = rb.astype(T), cf.astype(T)
    with np.errstate(all="ignore"):
        K = knee_world(st, tables, knee, T)
        H, Fp = rb[:, thighs, 0:3].astype(T), rb[:, feet, 0:3].astype(T)
        V = rb[:, feet, 7:9].astype(T)
        zero = np.zeros((N, 4), dtype=T)
        pens = []
        for A, E, ss in ((H, K, THIGH_S), (K, Fp, SHANK_S)):
            d = zero.copy()
            for s in ss:
                X = A + T(s) * (E - A)
                pen = (height(k, height_samples, X[..., 0], X[..., 1]) + c["body_radius"]) - X[..., 2]
                pens.append(pen)
                d = np.where(pen > d, pen, d)
            f = c["stiffness"] * d
            force = np.where(d > 0, np.where(f < c["max_force"], f, c["max_force"]), T(0))
            if A is H:
                d_thigh, F_thigh = d, force
            else:
                d_shank, F_shank = d, force
        sp = np.sqrt(V[..., 0] * V[..., 0] + V[..., 1] * V[..., 1])
        ex, ey = V[..., 0] / sp, V[..., 1] / sp
        rise = height(k, height_samples, Fp[..., 0] + ex * c["probe"], Fp[..., 1] + ey * c["probe"]) - Fp[..., 2]
        hit = (sp > c["min_speed"]) & (rise > c["stumble_height"])
        m = c["wall_damping"] * sp
        mag = np.where(m < c["max_force"], m, c["max_force"])
        fx, fy = np.where(hit, -(mag * ex), T(0)), np.where(hit, -(mag * ey), T(0))
    out_t = rb.dtype
    for l in range(4):
        rb[:, shanks[l], 0:3] = K[:, l].astype(out_t)
        cf[:, thighs[l]] = np.stack([zero[:, l], zero[:, l], F_thigh[:, l]], axis=1).astype(out_t)
        cf[:, shanks[l]] = np.stack([zero[:, l], zero[:, l], F_shank[:, l]], axis=1).astype(out_t)
        cf[:, feet[l], 0], cf[:, feet[l], 1] = fx[:, l].astype(out_t), fy[:, l].astype(out_t)
    leg = np.stack([d_thigh > 0, d_shank > 0], axis=2).reshape(N, 8).astype(np.uint8)
    if trace is not None:
        trace.update(K=K, d_thigh=d_thigh, d_shank=d_shank, F_thigh=F_thigh, F_shank=F_shank, speed=sp, rise=rise, hit=hit, mag=mag,
                     pens=np.stack(pens, axis=-1), fx=fx, fy=fy)
    return dict(contact_forces=cf, rigid_body_state=rb, leg_contact=leg, stumbled=hit.astype(np.uint8))
