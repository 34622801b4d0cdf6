"""TEST INFRASTRUCTURE: numpy float32 restatement of dtc_sim_step_tilt (csrc/sim.hip; include/dtc_hip.h states the operations): the
surrogate step of tests/sim_oracle.py with a body plane that follows the support points of the stance feet.  Every value below is one
single-rounded float32 operation in the kernel's order, sums over legs run in leg order from float32 0, so the kernel's outputs are
compared bit for bit.  This file is the specification of the tilt model.  Nothing here imports the package's kernels."""
import numpy as np

import sim_oracle as O
from sim_oracle import F, STATE, INPUTS  # noqa: F401


def config_dict(c, rows, cols, seed=0, counter=0):
    """sim_oracle.config_dict plus the two constants of DtcSimTilt."""
    return dict(O.config_dict(c, rows, cols, seed=seed, counter=counter), max_slope=F(c.max_slope), min_det=F(c.min_det))


def tilt_entries(nx, ny, nz):
    """The three entries of Rt (the minimal rotation that takes z to n) that are not +-n: Rt[0][0], Rt[0][1] = Rt[1][0], Rt[1][1]."""
    k1 = F(1) + nz
    return F(1) - (nx * nx) / k1, -((nx * ny) / k1), F(1) - (ny * ny) / k1


def rotate(R, n, v0, v1, v2):
    """Rt v.  `R`, `n`: per-env arrays (or arrays that broadcast against v)."""
    (r00, r01, r11), (nx, ny, nz) = R, n
    return (r00 * v0 + r01 * v1) + nx * v2, (r01 * v0 + r11 * v1) + ny * v2, (-(nx * v0) - ny * v1) + nz * v2


def rotate_t(R, n, v0, v1, v2):
    """Rt^T v."""
    (r00, r01, r11), (nx, ny, nz) = R, n
    return (r00 * v0 + r01 * v1) - nx * v2, (r01 * v0 + r11 * v1) - ny * v2, (nx * v0 + ny * v1) + nz * v2


def split_quaternion(q):
    """[N,4] (x, y, z, w) -> the yaw pair (zy, wy) and the body z-axis n in the yaw frame, both normalised."""
    qx, qy, qz, qw = (q[:, i].astype(F) for i in range(4))
    ry = np.sqrt(qz * qz + qw * qw)
    zy, wy = qz / ry, qw / ry
    c, s = F(1) - F(2) * (zy * zy), F(2) * (zy * wy)
    ax, ay, az = F(2) * (qx * qz + qw * qy), F(2) * (qy * qz - qw * qx), F(1) - F(2) * (qx * qx + qy * qy)      # R(q) z, world frame
    mx, my = c * ax + s * ay, c * ay - s * ax
    rn = np.sqrt((mx * mx + my * my) + az * az)
    return zy, wy, (mx / rn, my / rn, az / rn)


def sim_step(st, k, tables, actions, height_samples, u_cmd=None, trace=None):
    """One env step with tilt; arguments and result as sim_oracle.sim_step, `k` from config_dict above.  `trace` receives one dict
    per substep: the yaw-only step's entries with p, u in the yaw frame (r = Rt p, s = Rt u), plus n (before the substep's fit),
    n_new, wx, wy, stance and n_s (the legs of the fit), the slopes a, b as fitted (before the clamp), det and fit (whether the fit was
    taken)."""
    t = {name: np.asarray(v, dtype=F) for name, v in tables.items()}
    o = {name: np.array(st[name], copy=True) for name in STATE}
    N = actions.shape[0]
    dt, half_dt = k["sim_dt"], F(0.5) * k["sim_dt"]
    lo, hi, dflt = t["dof_pos_limits"][:, 0], t["dof_pos_limits"][:, 1], t["default_dof_pos"]
    J, nom, hip = t["leg_jacobian"], t["foot_nominal"], t["hip_offset"]
    a = np.minimum(np.maximum(actions.astype(F), -k["clip_actions"]), k["clip_actions"])
    goal = np.minimum(np.maximum(a * k["action_scale"] + dflt, lo), hi)
    q, qd = o["dof_pos"].astype(F), o["dof_vel"].astype(F)
    x, y, z = (o["root_states"][:, i].copy() for i in (0, 1, 2))
    zero = np.zeros(N, dtype=F)
    col = lambda v: v[:, None]                                                          # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        qz, qw, (nx, ny, nz) = split_quaternion(o["root_states"][:, 3:7])
        for _ in range(k["decimation"]):
            tau = O.pd_torque(k, t, st, goal, q, qd)
            qd = qd + (tau / k["joint_inertia"]) * dt
            q = q + qd * dt
            below = q < lo
            q, qd = np.where(below, lo, q), np.where(below, F(0), qd)
            above = q > hi
            q, qd = np.where(above, hi, q), np.where(above, F(0), qd)
            dq = (q - dflt).reshape(N, 4, 3)
            v = qd.reshape(N, 4, 3)
            p = nom[None] + ((J[None, :, :, 0] * dq[:, :, None, 0] + J[None, :, :, 1] * dq[:, :, None, 1]) + J[None, :, :, 2] * dq[:, :, None, 2])
            u = (J[None, :, :, 0] * v[:, :, None, 0] + J[None, :, :, 1] * v[:, :, None, 1]) + J[None, :, :, 2] * v[:, :, None, 2]
            # the tilt rotation: the feet in the yaw frame
            R, n = tuple(col(e) for e in tilt_entries(nx, ny, nz)), (col(nx), col(ny), col(nz))
            r = np.stack(rotate(R, n, p[:, :, 0], p[:, :, 1], p[:, :, 2]), axis=2)
            sv = np.stack(rotate(R, n, u[:, :, 0], u[:, :, 1], u[:, :, 2]), axis=2)
            c, s = F(1) - F(2) * (qz * qz), F(2) * (qz * qw)
            fx = col(x) + (col(c) * r[:, :, 0] - col(s) * r[:, :, 1])
            fy = col(y) + (col(s) * r[:, :, 0] + col(c) * r[:, :, 1])
            h = O.terrain_height(k, height_samples, fx, fy)
            bz = h[:, 0] - r[:, 0, 2]
            for l in range(1, 4):
                bz = np.maximum(bz, h[:, l] - r[:, l, 2])
            ct = ((col(bz) + r[:, :, 2]) - h) <= k["contact_eps"]
            nc = zero.copy()
            for l in range(4):
                nc = nc + np.where(ct[:, l], F(1), F(0))
            spx, spy, sux, suy = zero.copy(), zero.copy(), zero.copy(), zero.copy()
            for l in range(4):
                m = ct[:, l]
                spx, spy = np.where(m, spx + r[:, l, 0], spx), np.where(m, spy + r[:, l, 1], spy)
                sux, suy = np.where(m, sux + sv[:, l, 0], sux), np.where(m, suy + sv[:, l, 1], suy)
            pmx, pmy, umx, umy = spx / nc, spy / nc, sux / nc, suy / nc
            num, den = zero.copy(), zero.copy()
            for l in range(4):
                m = ct[:, l]
                dpx, dpy, dux, duy = r[:, l, 0] - pmx, r[:, l, 1] - pmy, sv[:, l, 0] - umx, sv[:, l, 1] - umy
                num = np.where(m, num + (dpx * duy - dpy * dux), num)
                den = np.where(m, den + (dpx * dpx + dpy * dpy), den)
            w = np.where(den > k["r_min"] * k["r_min"], -(num / den), F(0))
            vbx = (-umx) + w * pmy
            vby = (-umy) - w * pmx
            # the new tilt.  Stance legs: those extended to within contact_eps of the most extended one (body frame); centred least
            # squares of d = h - p.z over their body-frame xy, d relative to the first of them
            zmin = p[:, 0, 2]
            for l in range(1, 4):
                zmin = np.where(p[:, l, 2] < zmin, p[:, l, 2], zmin)
            sl = (p[:, :, 2] - col(zmin)) <= k["contact_eps"]
            ns = zero.copy()
            for l in range(4):
                ns = ns + np.where(sl[:, l], F(1), F(0))
            d = h - p[:, :, 2]
            d0 = np.where(sl[:, 0], d[:, 0], np.where(sl[:, 1], d[:, 1], np.where(sl[:, 2], d[:, 2], d[:, 3])))
            tpx, tpy, te = zero.copy(), zero.copy(), zero.copy()
            for l in range(4):
                m = sl[:, l]
                tpx, tpy, te = np.where(m, tpx + p[:, l, 0], tpx), np.where(m, tpy + p[:, l, 1], tpy), np.where(m, te + (d[:, l] - d0), te)
            mx, my, me = tpx / ns, tpy / ns, te / ns
            sxx, sxy, syy, sxe, sye = (zero.copy() for _ in range(5))
            for l in range(4):
                m = sl[:, l]
                dx, dy, de = p[:, l, 0] - mx, p[:, l, 1] - my, (d[:, l] - d0) - me
                sxx, sxy, syy = np.where(m, sxx + dx * dx, sxx), np.where(m, sxy + dx * dy, sxy), np.where(m, syy + dy * dy, syy)
                sxe, sye = np.where(m, sxe + dx * de, sxe), np.where(m, sye + dy * de, sye)
            det = sxx * syy - sxy * sxy
            sa = (sxe * syy - sye * sxy) / det
            sb = (sye * sxx - sxe * sxy) / det
            ms = k["max_slope"]
            ca = np.where(sa < -ms, -ms, np.where(sa > ms, ms, sa))
            cb = np.where(sb < -ms, -ms, np.where(sb > ms, ms, sb))
            rr = np.sqrt((ca * ca + cb * cb) + F(1))
            fit = (ns >= F(3)) & (det > k["min_det"])
            nnx, nny, nnz = np.where(fit, (-ca) / rr, nx), np.where(fit, (-cb) / rr, ny), np.where(fit, F(1) / rr, nz)
            wx, wy = -((nny - ny) / dt), (nnx - nx) / dt
            if trace is not None:
                trace.append(dict(tau=tau, q=q, qd=qd, p=r, u=sv, p_body=p, h=h, base_z=bz, contact=ct, n_c=nc, omega=w, vbx=vbx, vby=vby,
                                  c=c, s=s, n=np.stack([nx, ny, nz], axis=1), n_new=np.stack([nnx, nny, nnz], axis=1), wx=wx, wy=wy,
                                  a=sa, b=sb, det=det, fit=fit, stance=sl, n_s=ns, x=x, y=y))
            nx, ny, nz = nnx, nny, nnz
            x = x + (c * vbx - s * vby) * dt
            y = y + (s * vbx + c * vby) * dt
            vz = (bz - z) / dt
            z = bz
            ee = half_dt * w
            zn, wn = qz + ee * qw, qw - ee * qz
            rq = np.sqrt(zn * zn + wn * wn)
            qz, qw = zn / rq, wn / rq
            if trace is not None:
                trace[-1]["vz"] = vz

        # after the loop: the NEW yaw and the NEW tilt
        c, s = F(1) - F(2) * (qz * qz), F(2) * (qz * qw)
        Vx, Vy = c * vbx - s * vby, s * vbx + c * vby
        Wx, Wy = c * wx - s * wy, s * wx + c * wy
        R1, n1 = tilt_entries(nx, ny, nz), (nx, ny, nz)
        R, n = tuple(col(e) for e in R1), (col(nx), col(ny), col(nz))
        r = np.stack(rotate(R, n, p[:, :, 0], p[:, :, 1], p[:, :, 2]), axis=2)
        sv = np.stack(rotate(R, n, u[:, :, 0], u[:, :, 1], u[:, :, 2]), axis=2)
        k1 = F(1) + nz
        dn = np.sqrt(F(2) * k1)
        tx, ty, tw = (-ny) / dn, nx / dn, k1 / dn
        bl = rotate_t(R1, n1, vbx, vby, vz)
        ba = rotate_t(R1, n1, wx, wy, w)
        fz = k["weight"] / nc
    B, C, T = k["num_bodies"], k["num_commands"], k["buffer_len"]
    o["dof_pos"], o["dof_vel"], o["torques"], o["actions"] = q, qd, tau, a
    quat = [qw * tx - qz * ty, qw * ty + qz * tx, qz * tw, qw * tw]
    o["root_states"] = np.stack([x, y, z] + quat + [Vx, Vy, vz, Wx, Wy, w], axis=1)
    o["base_lin_vel"] = np.stack(bl, axis=1)
    o["last_base_ang_vel"] = np.array(st["base_ang_vel"], copy=True)
    o["base_ang_vel"] = np.stack(ba, axis=1)
    o["projected_gravity"] = np.stack([nx, ny, -nz], axis=1)
    o["base_quat"] = np.stack(quat, axis=1)
    o["base_pos"] = np.stack([x, y, z], axis=1)
    for l in range(4):
        r0, r1, r2 = r[:, l, 0], r[:, l, 1], r[:, l, 2]
        rx, ry, rz = (sv[:, l, 0] - w * r1) + wy * r2, (sv[:, l, 1] + w * r0) - wx * r2, sv[:, l, 2] + (wx * r1 - wy * r0)
        row = o["rigid_body_state"][:, k["feet"][l]]
        row[:, 0] = x + (c * r0 - s * r1)
        row[:, 1] = y + (s * r0 + c * r1)
        row[:, 2] = z + r2
        row[:, 7] = Vx + (c * rx - s * ry)
        row[:, 8] = Vy + (s * rx + c * ry)
        row[:, 9] = vz + rz
        t0, t1, t2 = rotate(R1, n1, hip[l, 0], hip[l, 1], hip[l, 2])
        row = o["rigid_body_state"][:, k["thighs"][l]]
        row[:, 0] = x + (c * t0 - s * t1)
        row[:, 1] = y + (s * t0 + c * t1)
        row[:, 2] = z + t2
    o["contact_forces"] = np.zeros((N, B, 3), dtype=F)
    for l in range(4):
        o["contact_forces"][:, k["feet"][l], 2] = np.where(ct[:, l], fz, F(0))

    elen = st["episode_length_buf"] + 1
    o["episode_length_buf"] = elen
    for name, new in (("lin_vel_buffer", np.stack([bl[0], bl[1]], axis=1)), ("ang_vel_buffer", ba[2][:, None]), ("cmd_buffer", st["commands"])):
        o[name][:-1] = st[name][1:]
        o[name][-1] = new
    due = elen % k["resampling_steps"] == 0
    ud = O.command_draws(k, N) if u_cmd is None else u_cmd.astype(F)
    (sx, lx), (sy, ly) = O._span(k["lin_vel_x"]), O._span(k["lin_vel_y"])
    s3, l3 = O._span(k["heading"] if k["heading_command"] else k["ang_vel_yaw"])
    cx, cy, third = sx * ud[:, 0] + lx, sy * ud[:, 1] + ly, s3 * ud[:, 2] + l3
    keep = np.where(np.sqrt(cx * cx + cy * cy) > F(0.1), F(1), F(0))
    cc = 3 if k["heading_command"] else 2
    o["commands"][:, cc] = np.where(due, third, st["commands"][:, cc])
    o["commands"][:, 0] = np.where(due, cx * keep, st["commands"][:, 0])
    o["commands"][:, 1] = np.where(due, cy * keep, st["commands"][:, 1])
    contact = np.stack([o["contact_forces"][:, k["feet"][l], 2] for l in range(4)], axis=1) > F(1)
    o["contact_filt"] = contact | st["last_contacts"].astype(bool)
    o["last_contacts"] = contact
    return o


# ------------------------------------------------------------------------------------------------ seeded cases (tests/sim_cases.py + a tilt)
def quaternion(yaw, ax, ay):
    """float32 [N,4] (x, y, z, w) = q_yaw (x) q_tilt for the body z-axis n ~ (ax, ay, 1) in the yaw frame, computed in float64."""
    yaw, ax, ay = (np.asarray(v, dtype=np.float64) for v in (yaw, ax, ay))
    n = np.stack([ax, ay, np.ones_like(ax)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = np.sqrt(2 * (1 + n[:, 2]))
    tx, ty, tw = -n[:, 1] / d, n[:, 0] / d, (1 + n[:, 2]) / d
    zy, wy = np.sin(yaw / 2), np.cos(yaw / 2)
    return np.stack([wy * tx - zy * ty, wy * ty + zy * tx, zy * tw, wy * tw], axis=1).astype(F)


def state(N, cfg, seed=51):
    """sim_cases.state with a whole quaternion: every third env level (the identity swing), the others tilted by slopes up to 0.3."""
    import sim_cases as CASES
    st = CASES.state(N, cfg, seed)
    g = np.random.default_rng(seed + 1000)
    yaw = 2 * np.arctan2(st["root_states"][:, 5].astype(np.float64), st["root_states"][:, 6].astype(np.float64))
    ax, ay = 0.3 * (2 * g.random(N) - 1), 0.3 * (2 * g.random(N) - 1)
    level = np.arange(N) % 3 == 1
    st["root_states"][:, 3:7] = quaternion(yaw, np.where(level, 0.0, ax), np.where(level, 0.0, ay))
    return st


def run(N, cfg, rough, steps=6, u_given=True, seed=0, trace=None, st=None, actions=None, hs=None):
    """`steps` chained oracle steps from state(N, cfg): [(actions, u_cmd, state after)], as sim_cases.run."""
    import sim_cases as CASES
    hs = CASES.terrain(rough) if hs is None else hs
    t = CASES.tables(cfg)
    st, out = state(N, cfg) if st is None else st, []
    for i in range(steps):
        a = CASES.actions(N, cfg, i) if actions is None else actions(i)
        u = CASES.draws(N, i) if u_given else None
        k = config_dict(cfg, hs.shape[0], hs.shape[1], seed=seed, counter=i)
        new = sim_step(st, k, t, a, hs, u, trace=trace)
        out.append((a, u, new))
        st = dict(st, **new)
    return out
