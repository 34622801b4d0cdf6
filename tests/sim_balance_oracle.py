"""TEST INFRASTRUCTURE: numpy restatement of dtc_sim_balance (csrc/sim_balance.hip; include/dtc_hip.h states the operations B1..B9),
operation by operation: with dtype float32 every value below is one single-rounded float32 operation in the kernel's order (add,
subtract, multiply, divide, sqrt and comparisons only, no libm call), so the kernel's outputs are compared bit for bit; with dtype
float64 the same rule runs in double for the property tests.  It is the specification.  Nothing here imports the library."""
import numpy as np

F = np.float32
ORDER = (0, 1, 3, 2)             # FL, FR, HR, HL: the legs (FL, FR, HL, HR) taken round the body
CONSTANTS = ("gravity", "h_min", "lean_eps", "fall_angle", "fall_force", "dt")
# the tensors the launch writes (all of them also read, except fallen)
WRITTEN = ("root_states", "base_pos", "base_quat", "projected_gravity", "base_lin_vel", "base_ang_vel", "rigid_body_state",
           "contact_forces", "lean", "fallen")
READ_ONLY = ("contact_filt", "episode_length_buf")


def balance_dict(b, sim_dt, decimation):
    """The constants of a dtc_amd.sim.BalanceConfig as the kernel receives them (float32 scalars); dt = float32(sim_dt * decimation)."""
    d = {name: F(getattr(b, name)) for name in CONSTANTS if name != "dt"}
    d["dt"] = F(float(sim_dt) * int(decimation))
    d["com_offset"] = (F(b.com_offset[0]), F(b.com_offset[1]))
    return d


def _rot(q, v, T):
    """rot(q, v) as C1 of dtc_sim_contacts: t = 2 * (qv x v); c = qv x t; rot.i = (v.i + q.w * t.i) + c.i.  q: four arrays, v: three."""
    qx, qy, qz, qw = q
    two = T(2)
    tx, ty, tz = two * (qy * v[2] - qz * v[1]), two * (qz * v[0] - qx * v[2]), two * (qx * v[1] - qy * v[0])
    cx, cy, cz = qy * tz - qz * ty, qz * tx - qx * tz, qx * ty - qy * tx
    return (v[0] + qw * tx) + cx, (v[1] + qw * ty) + cy, (v[2] + qw * tz) + cz


def balance(st, feet, bk, dtype=F, trace=None):
    """dtc_sim_balance on the state `st` a surrogate step left behind: root_states, base_pos, base_quat, projected_gravity,
    base_lin_vel, base_ang_vel, rigid_body_state, contact_forces, contact_filt [N,4], episode_length_buf [N] (as the step left it:
    1 in the step after a reset), lean [N,4].  `feet`: the four foot rows, leg order; `bk`: balance_dict.  Returns a dict of the
    tensors of WRITTEN: copies with the kernel's values; `st` is left unchanged.  `trace`, a dict, receives the branch record."""
    T = dtype
    c = {name: T(bk[name]) for name in CONSTANTS}
    ox, oy = T(bk["com_offset"][0]), T(bk["com_offset"][1])
    N = st["base_pos"].shape[0]
    out = {name: np.array(st[name], copy=True) for name in WRITTEN if name != "fallen"}
    if T != F:
        out = {name: a.astype(T) for name, a in out.items()}
    rb, cf, rs = out["rigid_body_state"], out["contact_forces"], out["root_states"]
    zero, one, half = T(0), T(1), T(0.5)
    with np.errstate(all="ignore"):
        B = out["base_pos"].copy()
        q = tuple(out["base_quat"][:, i].copy() for i in range(4))
        fresh = st["episode_length_buf"] == 1
        px, py, vx, vy = (out["lean"][:, i].copy() for i in range(4))
        # B1. the stance feet in the order FL, FR, HR, HL, packed to the front: V[0 .. k - 1]
        cnt = np.zeros(N, dtype=np.int64)
        V = [[np.zeros(N, dtype=T) for _ in range(3)] for _ in range(4)]
        for l in ORDER:
            s = st["contact_filt"][:, l] != 0
            P = [rb[:, feet[l], i].astype(T) for i in range(3)]
            for slot in range(4):
                put = s & (cnt == slot)
                for i in range(3):
                    V[slot][i] = np.where(put, P[i], V[slot][i])
            cnt = cnt + s
        k = cnt
        # B2. the centre of mass over the ground: the base's xy plus com_offset turned by the yaw of base_quat
        ry = np.sqrt(q[2] * q[2] + q[3] * q[3])
        zy, wy = q[2] / ry, q[3] / ry
        cy_, sy_ = one - T(2) * (zy * zy), T(2) * (zy * wy)
        cx = B[:, 0] + (cy_ * ox - sy_ * oy)
        cyy = B[:, 1] + (sy_ * ox + cy_ * oy)
        # B3. the nearest point of the support's boundary, edge by edge, and the side of every edge the centre lies on
        best = np.full(N, np.inf, dtype=T)
        nx, ny = V[0][0].copy(), V[0][1].copy()
        interior = np.zeros(N, dtype=bool)
        area = (V[1][0] - V[0][0]) * (V[2][1] - V[0][1]) - (V[1][1] - V[0][1]) * (V[2][0] - V[0][0])
        area = np.where(k == 4, area + ((V[2][0] - V[0][0]) * (V[3][1] - V[0][1]) - (V[2][1] - V[0][1]) * (V[3][0] - V[0][0])), area)
        left, right = np.ones(N, dtype=bool), np.ones(N, dtype=bool)
        for j in range(4):
            if j < 3:
                last = k == j + 1
                Ex, Ey = np.where(last, V[0][0], V[j + 1][0]), np.where(last, V[0][1], V[j + 1][1])
            else:
                Ex, Ey = V[0][0], V[0][1]
            active = (k >= 2) & (j < np.where(k == 2, 1, k)) if j > 0 else (k >= 1)     # edge 0 of a single foot: the point itself
            ex, ey = Ex - V[j][0], Ey - V[j][1]
            wx, wy_ = cx - V[j][0], cyy - V[j][1]
            ee = ex * ex + ey * ey
            t = (wx * ex + wy_ * ey) / ee
            t = np.where(t > zero, np.where(t < one, t, one), zero)                        # a NaN (ee == 0: one foot) gives 0
            gx, gy = V[j][0] + t * ex, V[j][1] + t * ey
            rx, ry_ = cx - gx, cyy - gy
            d2 = rx * rx + ry_ * ry_
            take = active & (d2 < best)
            best = np.where(take, d2, best)
            nx, ny = np.where(take, gx, nx), np.where(take, gy, ny)
            interior = np.where(take, (t > zero) & (t < one), interior)
            cr = ex * wy_ - ey * wx
            left, right = left & (~active | (cr >= zero)), right & (~active | (cr <= zero))
        inside = (k >= 3) & (((area > zero) & left) | ((area < zero) & right))
        dist = np.sqrt(best)
        d = np.where(inside, -dist, dist)
        ux, uy = (cx - nx) / dist, (cyy - ny) / dist
        # B4. the pendulum's length: the base over the highest stance foot, floored
        top = V[0][2].copy()
        for slot in range(1, 4):
            top = np.where((k > slot) & (V[slot][2] > top), V[slot][2], top)
        h0 = B[:, 2] - top
        h = np.where(h0 > c["h_min"], h0, c["h_min"])
        # B5. the acceleration of the lean
        den = h * h + d * d
        out_x, out_y = (c["gravity"] * (d * ux + h * px)) / den, (c["gravity"] * (d * uy + h * py)) / den
        m0 = np.sqrt(px * px + py * py)
        gin = c["gravity"] * (-d)
        in_x, in_y = -((gin * px) / (m0 * den)), -((gin * py) / (m0 * den))
        outside = (k >= 1) & (d > zero)
        within = (k >= 1) & ~outside
        restoring = within & (m0 > zero)
        ax = np.where(outside, out_x, np.where(restoring, in_x, zero))
        ay = np.where(outside, out_y, np.where(restoring, in_y, zero))
        # B6. semi-implicit Euler, then the landing and the step after a reset
        v1x, v1y = vx + ax * c["dt"], vy + ay * c["dt"]
        p1x, p1y = px + v1x * c["dt"], py + v1y * c["dt"]
        dot = p1x * px + p1y * py
        m1 = np.sqrt(p1x * p1x + p1y * p1y)
        by_sign = dot <= zero
        by_eps = m1 < c["lean_eps"]
        lands = within & (~(m0 > zero) | by_sign | by_eps)
        clear = lands | fresh
        p1x, p1y, v1x, v1y = (np.where(clear, zero, a) for a in (p1x, p1y, v1x, v1y))
        # B7. the fall
        m = np.sqrt(p1x * p1x + p1y * p1y)
        fell = m > c["fall_angle"]
        f0 = cf[:, 0, 2].astype(T)
        cf[:, 0, 2] = np.where(fell, np.where(f0 < c["fall_force"], c["fall_force"], f0), f0)
        # B8. the lean's rotation L = normalise(-p.y / 2, p.x / 2, 0, 1) about z x p, composed on the left: q' = L (x) q
        lx, ly = -(p1y * half), p1x * half
        ln = np.sqrt((lx * lx + ly * ly) + one)
        Lx, Ly, Lw = lx / ln, ly / ln, one / ln
        qn = (((Lw * q[0] + Lx * q[3]) + Ly * q[2]), ((Lw * q[1] - Lx * q[2]) + Ly * q[3]),
              ((Lw * q[2] + Lx * q[1]) - Ly * q[0]), ((Lw * q[3] - Lx * q[0]) - Ly * q[1]))
        qc = (-qn[0], -qn[1], -qn[2], qn[3])
        zeros = np.zeros(N, dtype=T)
        g = _rot(qc, (zeros, zeros, zeros - one), T)
        lv = _rot(qc, _rot(q, tuple(out["base_lin_vel"][:, i] for i in range(3)), T), T)
        wv = _rot(q, tuple(out["base_ang_vel"][:, i] for i in range(3)), T)
        av = _rot(qc, (wv[0] + (-v1y), wv[1] + v1x, wv[2]), T)
        z1 = B[:, 2] - (h * (m * m)) * half
        on = m > zero                                                                      # no lean: every value keeps the step's bits
    for i in range(4):
        out["base_quat"][:, i] = np.where(on, qn[i], q[i])
        rs[:, 3 + i] = np.where(on, qn[i], rs[:, 3 + i])
        rb[:, 0, 3 + i] = out["base_quat"][:, i]
    for i in range(3):
        out["projected_gravity"][:, i] = np.where(on, g[i], out["projected_gravity"][:, i])
        out["base_lin_vel"][:, i] = np.where(on, lv[i], out["base_lin_vel"][:, i])
        out["base_ang_vel"][:, i] = np.where(on, av[i], out["base_ang_vel"][:, i])
    rs[:, 10] = np.where(on, rs[:, 10] + (-v1y), rs[:, 10])
    rs[:, 11] = np.where(on, rs[:, 11] + v1x, rs[:, 11])
    zz = np.where(on, z1, B[:, 2])
    out["base_pos"][:, 2] = zz
    rs[:, 2] = np.where(on, z1, rs[:, 2])
    rb[:, 0, 0], rb[:, 0, 1], rb[:, 0, 2] = B[:, 0], B[:, 1], zz
    out["lean"] = np.stack([p1x, p1y, v1x, v1y], axis=1).astype(out["lean"].dtype)
    out["fallen"] = fell.astype(np.uint8)
    if trace is not None:
        trace.update(k=k, area=area, inside=inside, outside=outside, within=within, interior=interior, restoring=restoring,
                     lands=lands & ~fresh, by_sign=within & (m0 > zero) & by_sign & ~fresh, by_eps=within & (m0 > zero) & ~by_sign & by_eps & ~fresh,
                     fresh=fresh, fell=fell, d=d, h=h, m=m, on=on, ux=ux, uy=uy, f0=f0)
    return out


BRANCHES = ("feet0", "feet1", "feet2", "feet3", "feet4", "triangle_ccw", "triangle_cw", "inside", "outside_edge", "outside_vertex",
            "restoring", "land_sign", "land_eps", "fresh", "fall", "crash_kept", "upright")


def branches(trace, rows=slice(None)):
    """How many envs of `rows` take each branch, from the trace of `balance`."""
    t = {k: np.asarray(v)[rows] for k, v in trace.items()}
    k, live = t["k"], ~t["fresh"]
    seen = {f"feet{i}": int((k == i).sum()) for i in range(5)}
    seen.update(triangle_ccw=int(((k == 3) & (t["area"] > 0)).sum()), triangle_cw=int(((k == 3) & (t["area"] < 0)).sum()),
                inside=int((t["inside"] & live).sum()), outside_edge=int((t["outside"] & t["interior"] & live & (k >= 2)).sum()),
                outside_vertex=int((t["outside"] & ~t["interior"] & live & (k >= 2)).sum()),
                restoring=int((t["restoring"] & ~t["lands"] & live).sum()), land_sign=int(t["by_sign"].sum()), land_eps=int(t["by_eps"].sum()),
                fresh=int(t["fresh"].sum()), fall=int(t["fell"].sum()), crash_kept=int((t["fell"] & (t["f0"] > 150)).sum()),
                upright=int((~t["on"] & np.isfinite(t["m"])).sum()))
    return seen


def run(st, feet, bk, steps, dtype=np.float64):
    """`steps` calls of `balance` on a scene that stands still: the step's tensors are `st`'s every time, only the lean is carried.
    Returns (lean [steps + 1, N, 4], fallen [steps, N]) in `dtype`."""
    lean = [np.asarray(st["lean"], dtype=dtype)]
    fallen = []
    for _ in range(steps):
        out = balance(dict(st, lean=lean[-1]), feet, bk, dtype)
        lean.append(out["lean"].astype(dtype))
        fallen.append(out["fallen"])
    return np.stack(lean), np.stack(fallen)
