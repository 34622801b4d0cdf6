"""TEST INFRASTRUCTURE: numpy float32 restatement of dtc_sim_step_fly (csrc/sim.hip; include/dtc_hip.h states the operations): the
surrogate step of tests/sim_oracle.py, tests/sim_tilt_oracle.py or tests/sim_actuator_oracle.py (either base) with a vertical degree
of freedom of the base: free flight under gravity, landing, and a crash where the support rises by more than max_step_up.  Every
value below is one single-rounded float32 operation in the kernel's order, sums over legs run in leg order from float32 0, so the
kernel's outputs are compared bit for bit.  This file is the specification of the flight model.  `dtype=np.float64` runs the same
recurrence, from the same float32 constants and inputs, in float64: the yardstick of the property tests
(tests/test_sim_flight_host.py).  Nothing here imports the package's kernels."""
import numpy as np

import sim_actuator_oracle as AO
import sim_oracle as O
import sim_tilt_oracle as TO
from sim_oracle import F, INPUTS  # noqa: F401

FLAGS = ("airborne", "crashed")


def state_names(act):
    return (AO.STATE if act else O.STATE) + FLAGS


def config_dict(c, rows, cols, seed=0, counter=0):
    """The constants of the step underneath (with c.actuator: sim_actuator_oracle's, else sim_tilt_oracle's, which holds
    sim_oracle's) plus those of DtcSimFlight (c.flight must be set)."""
    base = AO.config_dict if c.actuator is not None else TO.config_dict
    f = c.flight
    return dict(base(c, rows, cols, seed=seed, counter=counter), gravity=F(f.gravity), max_step_up=F(f.max_step_up), crash_force=F(f.crash_force))


def _heights(k, hs, fx, fy, D):
    wx = (fx + k["border_size"]) / k["horizontal_scale"]
    wy = (fy + k["border_size"]) / k["horizontal_scale"]
    cx = np.clip(np.trunc(wx).astype(np.int64), 0, k["rows"] - 2)
    cy = np.clip(np.trunc(wy).astype(np.int64), 0, k["cols"] - 2)
    h = np.minimum(np.minimum(hs[cx, cy], hs[cx + 1, cy]), hs[cx, cy + 1])
    return h.astype(D) * k["vertical_scale"]


def _split_quaternion(q, D):
    """sim_tilt_oracle.split_quaternion in the dtype D."""
    qx, qy, qz, qw = (q[:, i].astype(D) for i in range(4))
    ry = np.sqrt(qz * qz + qw * qw)
    zy, wy = qz / ry, qw / ry
    c, s = D(1) - D(2) * (zy * zy), D(2) * (zy * wy)
    ax, ay, az = D(2) * (qx * qz + qw * qy), D(2) * (qy * qz - qw * qx), D(1) - D(2) * (qx * qx + qy * qy)
    mx, my = c * ax + s * ay, c * ay - s * ax
    rn = np.sqrt((mx * mx + my * my) + az * az)
    return zy, wy, (mx / rn, my / rn, az / rn)


def _tilt_entries(nx, ny, nz, D):
    k1 = D(1) + nz
    return D(1) - (nx * nx) / k1, -((nx * ny) / k1), D(1) - (ny * ny) / k1


def sim_step(st, k, tables, actions, height_samples, u_cmd=None, trace=None, *, tilt=False, act=False, lag_choice=None, u_push=None,
             push=False, dtype=F):
    """One env step with flight.  `st`: state_names(act) + INPUTS (airborne and crashed are outputs only); `k` from config_dict above;
    `act`: the step underneath is dtc_sim_step_act (`lag_choice`, `u_push`, `push` as in sim_actuator_oracle.sim_step).  Returns the
    new state dict.  `trace` receives one dict per substep: air, crashed (sticky), base_z, z, vz, x, y, Vw (the world planar
    velocity), omega, contact, n_c (as left by the substep), vzb, zb, vzg, and with tilt n (as left) and wx, wy."""
    D = dtype
    t = {name: np.asarray(v, dtype=F).astype(D) for name, v in tables.items()}
    k = {name: (D(v) if isinstance(v, np.floating) else v) for name, v in k.items()}
    names = state_names(act)
    o = {name: np.array(st[name], copy=True) for name in names if name not in FLAGS}
    inp = {name: np.asarray(st[name]).astype(D) for name in INPUTS}
    N = actions.shape[0]
    dec = k["decimation"]
    dt, half_dt = k["sim_dt"], D(0.5) * k["sim_dt"]
    lo, hi, dflt = t["dof_pos_limits"][:, 0], t["dof_pos_limits"][:, 1], t["default_dof_pos"]
    J, nom, hip = t["leg_jacobian"], t["foot_nominal"], t["hip_offset"]
    a = np.minimum(np.maximum(actions.astype(D), -k["clip_actions"]), k["clip_actions"])
    goal0 = np.minimum(np.maximum(a * k["action_scale"] + dflt, lo), hi)
    zero = np.zeros(N, dtype=D)
    if act:
        assert lag_choice is not None and len(lag_choice) == dec and all(0 <= int(c) <= 5 for c in lag_choice)
        lag = o["lag_state"].astype(D).copy()
    px, py = zero.copy(), zero.copy()
    if act and k["push"]:
        px, py = o["push_vel"][:, 0].astype(D).copy(), o["push_vel"][:, 1].astype(D).copy()
    q, qd = o["dof_pos"].astype(D), o["dof_vel"].astype(D)
    root = o["root_states"].astype(D)
    x, y, z = (root[:, i].copy() for i in (0, 1, 2))
    Vwx, Vwy, vz, w = root[:, 7].copy(), root[:, 8].copy(), root[:, 9].copy(), root[:, 12].copy()      # the carried state
    fresh = np.asarray(st["episode_length_buf"]) == 0
    crashed = np.zeros(N, dtype=bool)
    gdt = k["gravity"] * dt
    col = lambda v: v[:, None]                                                          # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if tilt:
            qz, qw, (nx, ny, nz) = _split_quaternion(root[:, 3:7], D)
        else:
            qz, qw = root[:, 5].copy(), root[:, 6].copy()
        wx = wy = zero
        for it in range(dec):
            goal = goal0
            if act:                                                                       # L1..L3
                lag[:, :5] = lag[:, 1:].copy()
                lag[:, 5] = a * k["action_scale"]
                if k["lag"]:
                    goal = np.minimum(np.maximum(lag[:, int(lag_choice[it])] + dflt, lo), hi)
            kp, kd = t["p_gains"] * inp["Kp_factors"], t["d_gains"] * inp["Kd_factors"]
            tau = ((kp * ((goal - q) + inp["motor_offsets"])) - kd * qd) * inp["motor_strengths"]
            tau = np.minimum(np.maximum(tau, -t["torque_limits"]), t["torque_limits"])
            qd = qd + (tau / k["joint_inertia"]) * dt
            q = q + qd * dt
            below = q < lo
            q, qd = np.where(below, lo, q), np.where(below, D(0), qd)
            above = q > hi
            q, qd = np.where(above, hi, q), np.where(above, D(0), qd)
            dq = (q - dflt).reshape(N, 4, 3)
            v = qd.reshape(N, 4, 3)
            p = nom[None] + ((J[None, :, :, 0] * dq[:, :, None, 0] + J[None, :, :, 1] * dq[:, :, None, 1]) + J[None, :, :, 2] * dq[:, :, None, 2])
            u = (J[None, :, :, 0] * v[:, :, None, 0] + J[None, :, :, 1] * v[:, :, None, 1]) + J[None, :, :, 2] * v[:, :, None, 2]
            if tilt:
                R, n = tuple(col(e) for e in _tilt_entries(nx, ny, nz, D)), (col(nx), col(ny), col(nz))
                r = np.stack(TO.rotate(R, n, p[:, :, 0], p[:, :, 1], p[:, :, 2]), axis=2)
                sv = np.stack(TO.rotate(R, n, u[:, :, 0], u[:, :, 1], u[:, :, 2]), axis=2)
            else:
                r, sv = p, u
            c, s = D(1) - D(2) * (qz * qz), D(2) * (qz * qw)
            fx = col(x) + (col(c) * r[:, :, 0] - col(s) * r[:, :, 1])
            fy = col(y) + (col(s) * r[:, :, 0] + col(c) * r[:, :, 1])
            h = _heights(k, height_samples, fx, fy, D)
            bz = h[:, 0] - r[:, 0, 2]
            for l in range(1, 4):
                bz = np.maximum(bz, h[:, l] - r[:, l, 2])
            ct = ((col(bz) + r[:, :, 2]) - h) <= k["contact_eps"]
            nc = zero.copy()
            for l in range(4):
                nc = nc + np.where(ct[:, l], D(1), D(0))
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
            wg = np.where(den > k["r_min"] * k["r_min"], -(num / den), D(0))
            vbx = (-umx) + wg * pmy
            vby = (-umy) - wg * pmx
            if tilt:                                                                      # T2, T3
                zmin = p[:, 0, 2]
                for l in range(1, 4):
                    zmin = np.where(p[:, l, 2] < zmin, p[:, l, 2], zmin)
                sl = (p[:, :, 2] - col(zmin)) <= k["contact_eps"]
                ns = zero.copy()
                for l in range(4):
                    ns = ns + np.where(sl[:, l], D(1), D(0))
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
                rr = np.sqrt((ca * ca + cb * cb) + D(1))
                fit = (ns >= D(3)) & (det > k["min_det"])
                nnx, nny, nnz = np.where(fit, (-ca) / rr, nx), np.where(fit, (-cb) / rr, ny), np.where(fit, D(1) / rr, nz)
                wxg, wyg = -((nny - ny) / dt), (nnx - nx) / dt
            # P1: a pending push rides on the grounded twist
            pushed = (px != D(0)) | (py != D(0))
            vbx = np.where(pushed, vbx + (c * px + s * py), vbx)
            vby = np.where(pushed, vby + (c * py - s * px), vby)
            # F1, F2: the ballistic candidate and the airborne test
            vzb = vz - gdt
            zb = z + vzb * dt
            air = (zb - bz) > k["contact_eps"]
            # F3: the take-off velocity of a grounded substep
            suz = zero.copy()
            for l in range(4):
                suz = np.where(ct[:, l], suz + sv[:, l, 2], suz)
            vzg = -(suz / nc)
            # F4: the crash
            crashed = crashed | (~air & ((bz - z) > k["max_step_up"]) & ~fresh)
            # F5: the selects
            Vwx, Vwy = np.where(air, Vwx, c * vbx - s * vby), np.where(air, Vwy, s * vbx + c * vby)
            w = np.where(air, w, wg)
            vz = np.where(air, vzb, vzg)
            z = np.where(air, zb, bz)
            nc = np.where(air, D(0), nc)
            ct = ct & ~col(air)
            if tilt:
                nx, ny, nz = np.where(air, nx, nnx), np.where(air, ny, nny), np.where(air, nz, nnz)
                wx, wy = np.where(air, D(0), wxg), np.where(air, D(0), wyg)
            # F6: the base moves
            x = x + Vwx * dt
            y = y + Vwy * dt
            ee = half_dt * w
            zn, wn = qz + ee * qw, qw - ee * qz
            rq = np.sqrt(zn * zn + wn * wn)
            qz, qw = zn / rq, wn / rq
            # P2, P3
            if act:
                px, py = px * k["keep"], py * k["keep"]
                small = (px * px + py * py) < k["floor2"]
                px, py = np.where(small, D(0), px), np.where(small, D(0), py)
            if trace is not None:
                sub = dict(air=air, crashed=crashed.copy(), base_z=bz, z=z, vz=vz, x=x, y=y, Vw=np.stack([Vwx, Vwy], axis=1), omega=w,
                           contact=ct, n_c=nc, vzb=vzb, zb=zb, vzg=vzg, q=q, qd=qd, h=h, p=r, u=sv)
                if tilt:
                    sub.update(n=np.stack([nx, ny, nz], axis=1), wx=wx, wy=wy)
                trace.append(sub)

        # after the loop: the NEW yaw (and the NEW tilt)
        c, s = D(1) - D(2) * (qz * qz), D(2) * (qz * qw)
        Vx, Vy = np.where(air, Vwx, c * vbx - s * vby), np.where(air, Vwy, s * vbx + c * vby)
        vbx, vby = np.where(air, c * Vwx + s * Vwy, vbx), np.where(air, c * Vwy - s * Vwx, vby)
        fz = np.where(air, D(0), k["weight"] / nc)
        if tilt:
            Wx, Wy = c * wx - s * wy, s * wx + c * wy
            R1, n1 = _tilt_entries(nx, ny, nz, D), (nx, ny, nz)
            R, n = tuple(col(e) for e in R1), (col(nx), col(ny), col(nz))
            r = np.stack(TO.rotate(R, n, p[:, :, 0], p[:, :, 1], p[:, :, 2]), axis=2)
            sv = np.stack(TO.rotate(R, n, u[:, :, 0], u[:, :, 1], u[:, :, 2]), axis=2)
            k1 = D(1) + nz
            dn = np.sqrt(D(2) * k1)
            tx, ty, tw = (-ny) / dn, nx / dn, k1 / dn
            bl = TO.rotate_t(R1, n1, vbx, vby, vz)
            ba = TO.rotate_t(R1, n1, wx, wy, w)
            quat = [qw * tx - qz * ty, qw * ty + qz * tx, qz * tw, qw * tw]
            pg = [nx, ny, -nz]
        else:
            Wx, Wy, r, sv = zero, zero, p, u
            bl, ba = (vbx, vby, vz), (zero, zero, w)
            quat = [zero, zero, qz, qw]
            pg = [zero, zero, zero - D(1)]
        rvx, rvy = Vx, Vy
        if act and k["push"] and push:                                                    # N1, N2
            ud = AO.push_draws(k, N) if u_push is None else u_push
            ud = ud.astype(D)
            px, py = k["push_span"] * ud[:, 0] + k["push_lo"], k["push_span"] * ud[:, 1] + k["push_lo"]
            rvx, rvy = px, py
    B = k["num_bodies"]
    if act:
        o["lag_state"] = lag
        if k["push"]:
            o["push_vel"] = np.stack([px, py], axis=1)
    o["dof_pos"], o["dof_vel"], o["torques"], o["actions"] = q, qd, tau, a
    o["root_states"] = np.stack([x, y, z] + quat + [rvx, rvy, vz, Wx, Wy, w], axis=1)
    o["base_lin_vel"] = np.stack(bl, axis=1)
    o["last_base_ang_vel"] = np.array(st["base_ang_vel"], copy=True).astype(D)
    o["base_ang_vel"] = np.stack(ba, axis=1)
    o["projected_gravity"] = np.stack(pg, axis=1)
    o["base_quat"] = np.stack(quat, axis=1)
    o["base_pos"] = np.stack([x, y, z], axis=1)
    o["rigid_body_state"] = o["rigid_body_state"].astype(D)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(4):
            r0, r1, r2 = r[:, l, 0], r[:, l, 1], r[:, l, 2]
            if tilt:
                rx, ry, rz = (sv[:, l, 0] - w * r1) + wy * r2, (sv[:, l, 1] + w * r0) - wx * r2, sv[:, l, 2] + (wx * r1 - wy * r0)
                t0, t1, t2 = TO.rotate(R1, n1, hip[l, 0], hip[l, 1], hip[l, 2])
            else:
                rx, ry, rz = sv[:, l, 0] - w * r1, sv[:, l, 1] + w * r0, sv[:, l, 2]
                t0, t1, t2 = hip[l, 0], hip[l, 1], hip[l, 2]
            row = o["rigid_body_state"][:, k["feet"][l]]
            row[:, 0] = x + (c * r0 - s * r1)
            row[:, 1] = y + (s * r0 + c * r1)
            row[:, 2] = z + r2
            row[:, 7] = Vx + (c * rx - s * ry)
            row[:, 8] = Vy + (s * rx + c * ry)
            row[:, 9] = vz + rz
            row = o["rigid_body_state"][:, k["thighs"][l]]
            row[:, 0] = x + (c * t0 - s * t1)
            row[:, 1] = y + (s * t0 + c * t1)
            row[:, 2] = z + t2
    o["contact_forces"] = np.zeros((N, B, 3), dtype=D)
    for l in range(4):
        o["contact_forces"][:, k["feet"][l], 2] = np.where(ct[:, l], fz, D(0))
    o["contact_forces"][:, 0, 2] = np.where(crashed, k["crash_force"], o["contact_forces"][:, 0, 2])
    o["airborne"], o["crashed"] = air.astype(np.uint8), crashed.astype(np.uint8)

    elen = st["episode_length_buf"] + 1
    o["episode_length_buf"] = elen
    for name, new in (("lin_vel_buffer", np.stack([bl[0], bl[1]], axis=1)), ("ang_vel_buffer", ba[2][:, None]), ("cmd_buffer", st["commands"])):
        o[name] = o[name].astype(D)
        o[name][:-1] = st[name][1:]
        o[name][-1] = new
    due = elen % k["resampling_steps"] == 0
    ud = (O.command_draws(k, N) if u_cmd is None else u_cmd).astype(D)
    rng = lambda v: (D(F(v[1] - v[0])), D(F(v[0])))                                      # noqa: E731  (sim_oracle._span)
    (sx, lx), (sy, ly) = rng(k["lin_vel_x"]), rng(k["lin_vel_y"])
    s3, l3 = rng(k["heading"] if k["heading_command"] else k["ang_vel_yaw"])
    cx, cy, third = sx * ud[:, 0] + lx, sy * ud[:, 1] + ly, s3 * ud[:, 2] + l3
    keep = np.where(np.sqrt(cx * cx + cy * cy) > D(F(0.1)), D(1), D(0))
    cc = 3 if k["heading_command"] else 2
    o["commands"] = o["commands"].astype(D)
    o["commands"][:, cc] = np.where(due, third, st["commands"][:, cc])
    o["commands"][:, 0] = np.where(due, cx * keep, st["commands"][:, 0])
    o["commands"][:, 1] = np.where(due, cy * keep, st["commands"][:, 1])
    contact = np.stack([o["contact_forces"][:, k["feet"][l], 2] for l in range(4)], axis=1) > D(1)
    o["contact_filt"] = contact | st["last_contacts"].astype(bool)
    o["last_contacts"] = contact
    return o


# ------------------------------------------------------------------------------------------------ the seeded fixture of the GPU test
STEPS = 6
PUSH_STEPS = (1, 2)
GROUND = 0.28                   # about the base height of the default pose over its support


def flight(**kw):
    from dtc_amd import sim as SIM
    return SIM.FlightConfig(**kw)


def config(decimation, tilt=False, act=False, **fly):
    import sim_cases as CASES
    return CASES.config(decimation, tilt=tilt, actuator=AO.actuator() if act else None, flight=flight(**fly))


def cell(v):
    """Table index of the world coordinate v (20 m border, 0.05 m cells)."""
    return int(round((v + 20.0) / 0.05))


def terrain():
    """A flat table of sim_cases' size with three features: a field of 0.4 m x 0.4 m holes 1.5 m deep on a 0.8 m pitch (x in
    [22, 26) m), a ledge (the ground lies 1 m lower for x in [27, 30)), and a wall (the ground lies 0.6 m higher from x = 30 m on)."""
    import sim_cases as CASES
    hs = np.zeros((CASES.ROWS, CASES.COLS), dtype=np.int16)
    for i in range(cell(22.0), cell(26.0), 16):
        for j in range(0, hs.shape[1] - 8, 16):
            hs[i:i + 8, j:j + 8] = -300
    hs[cell(27.0):cell(30.0)] = -200
    hs[cell(30.0):] = 120
    return hs


def state(N, cfg, seed=51):
    """The state of the step underneath (sim_cases / sim_tilt_oracle / sim_actuator_oracle: x in [20, 30) m, so over the flat, the
    holes and the low ground behind the ledge; z in [0.3, 0.4) m, so a little above the flat and 1.3 m above the low ground) with
    finite root velocities, the carried state.  From env 2 on, every fourth env is placed: level, 0.15 m above its standing height
    over the low ground and 0.05..0.1 m short of the point where its front feet reach the wall, flying at it with 2 m/s; and every
    fourth, offset by two, stands on the flat, its base at standing height.  The wall envs are in the default pose and have
    episode_length_buf >= 1, except the last of them from three on, which meets the wall in the step after a reset.  A single env
    (N = 1) is a wall env."""
    import sim_cases as CASES
    st = AO.state(N, cfg, seed) if cfg.actuator is not None else (TO.state(N, cfg, seed) if cfg.tilt else CASES.state(N, cfg, seed))
    g = np.random.default_rng(seed + 3000)
    root = st["root_states"]
    root[:, 7:13] = 0
    root[:, 7:9] = (0.3 * g.standard_normal((N, 2))).astype(F)
    root[:, 9] = (0.2 * g.standard_normal(N)).astype(F)
    root[:, 12] = (0.3 * g.standard_normal(N)).astype(F)
    if not cfg.tilt:
        root[:, 3:5] = 0
    walls = list(range(2, N, 4)) if N > 1 else [0]                  # a single env takes every branch itself
    for n in walls:
        root[n, 0], root[n, 1], root[n, 2] = 29.75 + 0.05 * g.random(), 20.5 + 4 * g.random(), -1.0 + GROUND + 0.15
        root[n, 3:7], root[n, 7:10], root[n, 12] = (0, 0, 0, 1), (2.0, 0, 0), 0
        st["dof_pos"][n], st["dof_vel"][n] = CASES.tables(cfg)["default_dof_pos"], 0     # feet under the hips: the front pair 0.17 m ahead
        st["episode_length_buf"][n] = max(int(st["episode_length_buf"][n]), 1)
    if len(walls) >= 3:
        st["episode_length_buf"][walls[-1]] = 0
    for n in range(4, N, 4):
        root[n, 0], root[n, 1], root[n, 2] = 20.5 + g.random(), 20.5 + 4 * g.random(), GROUND
        root[n, 9] = 0
    st["airborne"] = np.full(N, 0xFF, dtype=np.uint8)
    st["crashed"] = np.full(N, 0xFF, dtype=np.uint8)
    return st


def run(N, cfg, steps=STEPS, u_given=True, seed=0, trace=None, st=None, hs=None, actions=None, dtype=F, push_steps=PUSH_STEPS):
    """`steps` chained oracle steps from state(N, cfg) over terrain(): [(actions, u_cmd, lag_choice or None, u_push or None, push,
    state after)]."""
    import sim_cases as CASES
    hs, t = terrain() if hs is None else hs, CASES.tables(cfg)
    act = cfg.actuator is not None
    st, out = state(N, cfg) if st is None else st, []
    for i in range(steps):
        a = CASES.actions(N, cfg, i) if actions is None else actions(i)
        u = CASES.draws(N, i) if u_given else None
        ch = AO.choices(cfg.decimation, i) if act else None
        push = act and i in push_steps
        up = AO.push_u(N, i) if (u_given and push) else None
        k = config_dict(cfg, hs.shape[0], hs.shape[1], seed=seed, counter=i)
        new = sim_step(st, k, t, a, hs, u, trace=trace, tilt=bool(cfg.tilt), act=act, lag_choice=ch, u_push=up, push=push, dtype=dtype)
        out.append((a, u, ch, up, push, new))
        st = dict(st, **new)
    return out
