"""The GRU recurrence on operand images (csrc/gru_h2i.hip, DTC_GRU_H2I=1) against the default per-step kernels (csrc/gru_s3.hip).

    python deep-tracking-control_amd/tools/gru_h2i_bench.py [--reps 20] [--errors]

T = 24, H = 512, R in {1024, 1473, 1536} (the recurrent mini-batch of 4096 envs), microseconds, median of `reps` timed calls after warm-up:
(1) per launch: the forward step (dtc_gru_step_fwd_s3 / dtc_gru_step_fwd_h2i) and the six chunks of dh += dgh W_hh
    (dtc_gru_dgrad_parts_s3 / dtc_gru_dgrad_parts_h2i), each timed over 24 back-to-back launches;
(2) per recurrence: ops.gru_fwd / gru_bwd against ops.gru_fwd_h2i / gru_bwd_h2i without and with the valid-row images (every slot
    valid), the gate kernel per launch = (backward - 24 chunk launches) / 24.
--errors: the largest error of every output against an fp64 recurrence on both paths (T = 24, R = 1473), as tests/test_hip_gru_h2i.py prints.
Run it under `rocprofv3 --kernel-trace --stats -- python ...` for per-kernel times.  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import _ffi, h2i, ops  # noqa: E402

DEV = "cuda:0"
f32 = torch.float32


def timed(fn, reps, inner=1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / inner)
    return round(statistics.median(times), 1)


def case(R, H=512, T=24, reps=20):
    lib = _ffi.lib()
    g = torch.Generator(device=DEV).manual_seed(R + H)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    gi, h0, W, b = rn(T, R, 3 * H), (0.5 * rn(R, H)).clamp(-1.9, 1.9), rn(3 * H, H) / H ** 0.5, 0.2 * rn(3 * H)
    dhs = 0.01 * rn(T, R, H)
    e = lambda *s: torch.empty(*s, device=DEV)
    hs, gates, hn, dgi, dh0 = e(T + 1, R, H), e(T, R, 3 * H), e(T, R, H), e(T, R, 3 * H), e(R, H)
    p, c, st = _ffi.ptr, lambda t: _ffi.cptr(t, f32), _ffi.stream
    out = dict(what="gru_h2i_us", T=T, R=R, H=H)
    # ---- single launches
    img = ops.workspace(max(int(lib.dtc_gru_s3_image_bytes(H)), int(lib.dtc_gru_h2i_image_bytes(H, 0))), DEV)
    part, dgh = e(6, R, H), rn(R, 3 * H)
    hpi, dghi = h2i.HImage.from_tensor(h0), h2i.HImage.from_tensor(dgh)
    _ffi.check(lib.dtc_gru_s3_image(c(W), p(img), H, 0, st()), "image")
    out["step_fwd_s3"] = timed(lambda: lib.dtc_gru_step_fwd_s3(c(h0), p(img), c(b), c(gi[0]), p(hs[1]), p(gates[0]), p(hn[0]), R, H, st()), reps, T)
    _ffi.check(lib.dtc_gru_s3_image(c(W), p(img), H, 1, st()), "image")
    out["dgrad_parts_s3"] = timed(lambda: lib.dtc_gru_dgrad_parts_s3(c(dgh), p(img), p(part), R * H, R, H, 6, st()), reps, T)
    _ffi.check(lib.dtc_gru_h2i_image(c(W), p(img), H, 0, st()), "image")
    out["step_fwd_h2i"] = timed(lambda: lib.dtc_gru_step_fwd_h2i(hpi.ptr(), c(h0), p(img), c(b), c(gi[0]), p(hs[1]), p(gates[0]), p(hn[0]), None,
                                                                 None, None, None, 0, None, None, R, H, st()), reps, T)
    _ffi.check(lib.dtc_gru_h2i_image(c(W), p(img), H, 1, st()), "image")
    out["dgrad_parts_h2i"] = timed(lambda: lib.dtc_gru_dgrad_parts_h2i(dghi.ptr(), p(img), p(part), R * H, R, H, 6, st()), reps, T)
    # ---- whole recurrences
    ws = ops.workspace(ops.gru_workspace_bytes(T, R, H), DEV)
    lib.dtc_set_gru_seq(0)
    out["fwd_default"] = timed(lambda: ops.gru_fwd(gi, h0, W, b, hs, gates, hn, ws), reps)
    out["bwd_default"] = timed(lambda: ops.gru_bwd(dhs, hs, gates, hn, W, dgi, None, None, dh0, ws), reps)
    lib.dtc_set_gru_seq(-1)
    wsi = ops.workspace(ops.gru_h2i_workspace_bytes(T, R, H), DEV)
    out["fwd_h2i"] = timed(lambda: ops.gru_fwd_h2i(gi, h0, W, b, hs, gates, hn, wsi), reps)
    out["bwd_h2i"] = timed(lambda: ops.gru_bwd_h2i(dhs, hs, gates, hn, W, dgi, dh0, wsi), reps)
    M = T * R
    slot = torch.arange(M, dtype=torch.int32, device=DEV)
    im = {k: h2i.HImage(M, w * H, DEV) for k, w in (("hx", 1), ("hp", 1), ("drz", 2), ("dnh", 1), ("dni", 1))}
    out["fwd_h2i_images"] = timed(lambda: ops.gru_fwd_h2i(gi, h0, W, b, hs, gates, hn, wsi, slot, im["hx"], im["hp"]), reps)
    out["bwd_h2i_images"] = timed(lambda: ops.gru_bwd_h2i(dhs, hs, gates, hn, W, dgi, dh0, wsi, slot, im["drz"], im["dnh"], im["dni"]), reps)
    out["gate_bwd_default"] = round((out["bwd_default"] - T * out["dgrad_parts_s3"]) / T, 1)
    out["gate_bwd_h2i"] = round((out["bwd_h2i"] - T * out["dgrad_parts_h2i"]) / T, 1)
    out["gate_bwd_h2i_images"] = round((out["bwd_h2i_images"] - T * out["dgrad_parts_h2i"]) / T, 1)
    print(json.dumps(out), flush=True)


def errors(T=24, R=1473, H=512):
    g = torch.Generator(device=DEV).manual_seed(T * 1000 + R)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    gi, h0, W, b = rn(T, R, 3 * H), (0.5 * rn(R, H)).clamp(-1.9, 1.9), rn(3 * H, H) / H ** 0.5, 0.2 * rn(3 * H)
    dhs = 0.01 * rn(T, R, H)
    gi64, h064 = gi.double().requires_grad_(True), h0.double().requires_grad_(True)
    h, hsr, ghs = h064, [], []
    for t in range(T):
        gh = h @ W.double().T + b.double()
        gh.retain_grad()
        r, z = torch.sigmoid(gi64[t, :, :H] + gh[:, :H]), torch.sigmoid(gi64[t, :, H:2 * H] + gh[:, H:2 * H])
        h = (1 - z) * torch.tanh(gi64[t, :, 2 * H:] + r * gh[:, 2 * H:]) + z * h
        hsr.append(h)
        ghs.append(gh)
    (torch.stack(hsr) * dhs.double()).sum().backward()
    ref = dict(hs=torch.stack(hsr).detach(), dgi=gi64.grad, dh0=h064.grad, dgh=torch.stack([x.grad for x in ghs]))
    e = lambda *s: torch.empty(*s, device=DEV)
    out = dict(what="gru_h2i_errors", T=T, R=R, H=H)
    for name in ("default", "h2i"):
        hs, gates, hn, dgi, dh0 = e(T + 1, R, H), e(T, R, 3 * H), e(T, R, H), e(T, R, 3 * H), e(R, H)
        if name == "h2i":
            ws = ops.workspace(ops.gru_h2i_workspace_bytes(T, R, H), DEV)
            ops.gru_fwd_h2i(gi, h0, W, b, hs, gates, hn, ws)
            ops.gru_bwd_h2i(dhs, hs, gates, hn, W, dgi, dh0, ws)
            dgh = ops.gru_dgh_all_h2i(ws, T, R, H).view(T, R, 3 * H)
        else:
            ws = ops.workspace(ops.gru_workspace_bytes(T, R, H), DEV)
            ops.gru_fwd(gi, h0, W, b, hs, gates, hn, ws)
            ops.gru_bwd(dhs, hs, gates, hn, W, dgi, None, None, dh0, ws)
            dgh = ops.gru_dgh_all(ws, T, R, H).view(T, R, 3 * H)
        got = dict(hs=hs[1:], dgi=dgi, dh0=dh0, dgh=dgh)
        out[name] = {k: float(f"{float((got[k].double() - ref[k]).abs().max() / (1.0 if k == 'hs' else ref[k].abs().max())):.3e}") for k in ref}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--errors", action="store_true")
    a = ap.parse_args()
    for R in (1024, 1473, 1536):
        case(R, reps=a.reps)
    if a.errors:
        errors()
