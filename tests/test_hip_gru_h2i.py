"""GRU recurrence on operand images (csrc/gru_h2i.hip: dtc_gru_fwd_h2i / dtc_gru_bwd_h2i and their single-step entry points) against
fp64 references of torch.nn.GRU's recurrence -- the module the reference's `Memory` wraps (actor_critic_recurrent.py:92-116) over the
padded trajectories of utils/utils.py:33-70 --, next to the default kernels on the same inputs.  GPU only."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = torch.float32


def _inputs(T, R, H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(gi=rn(T, R, 3 * H), h0=(0.5 * rn(R, H)).clamp(-1.9, 1.9), W=rn(3 * H, H) / H ** 0.5, b=0.2 * rn(3 * H), dhs=0.01 * rn(T, R, H))


def _ref64(x):
    """torch.nn.GRU's recurrence (gate order r, z, n) and its gradients by autograd, in fp64 on the device."""
    gi, h0, dhs = x["gi"].double().requires_grad_(True), x["h0"].double().requires_grad_(True), x["dhs"].double()
    Wd, bd = x["W"].double(), x["b"].double()
    T, R, H3 = gi.shape
    H = H3 // 3
    h, hs, gates, hn, ghs = h0, [h0], [], [], []
    for t in range(T):
        gh = h @ Wd.T + bd
        gh.retain_grad()
        r, z = torch.sigmoid(gi[t, :, :H] + gh[:, :H]), torch.sigmoid(gi[t, :, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[t, :, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h)
        gates.append(torch.cat([r, z, n], 1))
        hn.append(gh[:, 2 * H:])
        ghs.append(gh)
    (torch.stack(hs[1:]) * dhs).sum().backward()
    return dict(hs=torch.stack(hs).detach(), gates=torch.stack(gates).detach(), hn=torch.stack(hn).detach(), dgi=gi.grad, dh0=h0.grad,
                dgh=torch.stack([g.grad for g in ghs]))


def _run(x, new, slot_row=None, M=0, images=False):
    """The whole recurrence, forward and backward, on the new path or the default one; every output pre-filled with NaN."""
    from dtc_amd import h2i, ops
    T, R, H3 = x["gi"].shape
    H = H3 // 3
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    o = dict(hs=nan(T + 1, R, H), gates=nan(T, R, 3 * H), hn=nan(T, R, H), dgi=nan(T, R, 3 * H), dh0=nan(R, H))
    if new:
        ws = ops.workspace(ops.gru_h2i_workspace_bytes(T, R, H), DEV)
        im = {}
        if images:
            im = {k: h2i.HImage(M, w * H, DEV) for k, w in (("hx", 1), ("hp", 1), ("drz", 2), ("dnh", 1), ("dni", 1), ("dgh", 3), ("dgi", 3))}
        ops.gru_fwd_h2i(x["gi"], x["h0"], x["W"], x["b"], o["hs"], o["gates"], o["hn"], ws, slot_row, im.get("hx"), im.get("hp"))
        ops.gru_bwd_h2i(x["dhs"], o["hs"], o["gates"], o["hn"], x["W"], o["dgi"], o["dh0"], ws, slot_row, im.get("drz"), im.get("dnh"),
                        im.get("dni"), im.get("dgh"), im.get("dgi"))
        o["dgh"] = ops.gru_dgh_all_h2i(ws, T, R, H).view(T, R, 3 * H).clone()
        o["images"] = im
    else:
        ws = ops.workspace(ops.gru_workspace_bytes(T, R, H), DEV)
        ops.gru_fwd(x["gi"], x["h0"], x["W"], x["b"], o["hs"], o["gates"], o["hn"], ws)
        ops.gru_bwd(x["dhs"], o["hs"], o["gates"], o["hn"], x["W"], o["dgi"], None, None, o["dh0"], ws)
        o["dgh"] = ops.gru_dgh_all(ws, T, R, H).view(T, R, 3 * H).clone()
    torch.cuda.synchronize()
    return o


FWD, BWD = ("hs", "gates", "hn"), ("dgi", "dh0", "dgh")


def _check_next_to_default(x, what):
    """Largest error of every output against fp64 on the new path and on the default path: forward err_new <= 2 err_default + 2e-6 (the
    persistent recurrence's bound), backward <= 2 err_default + 2e-7 of the tensor's largest element."""
    ref, new, old = _ref64(x), _run(x, True), _run(x, False)
    for k in FWD + BWD:
        scale = 1.0 if k in FWD else float(ref[k].abs().max())
        en, eo = (float((o[k].double() - ref[k]).abs().max()) / scale for o in (new, old))
        print(f"gru h2i {what} {k}: error vs fp64 new {en:.3e}, default {eo:.3e}" + ("" if k in FWD else f" (of the largest element {scale:.3e})"))
        assert np.isfinite(en), (k, "a slot nobody wrote, or a non-finite result")
        assert en <= 2.0 * eo + (2e-6 if k in FWD else 2e-7), (k, en, eo)
    return new


@pytest.mark.parametrize("H", [128, 256, 512])
@pytest.mark.parametrize("R", [1, 13, 129, 1473])
def test_step_kernels_vs_fp64(R, H):
    """The fused forward step and the data-gradient chunks through their own entry points, from packed images, against fp64, next to the
    single-pass fp32 kernels on the same inputs (the bounds of test_split_precision_step_kernels_vs_fp64)."""
    from dtc_amd import _ffi, h2i
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(R * 1000 + H)
    W = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(DEV)
    b = (0.2 * torch.randn(3 * H, generator=g)).to(DEV)
    hp = (0.5 * torch.randn(R, H, generator=g)).clamp(-1.9, 1.9).to(DEV)
    gi = torch.randn(R, 3 * H, generator=g).to(DEV)
    p, c = _ffi.ptr, lambda t: _ffi.cptr(t, f32)
    img = torch.empty(int(lib.dtc_gru_h2i_image_bytes(H, 0)) // 8 + 1, dtype=torch.float64, device=DEV)
    assert lib.dtc_gru_h2i_image_bytes(H, 0) >= lib.dtc_gru_h2i_image_bytes(H, 1) > 0
    outs = []
    for new in (False, True):
        h, gates, hn = (torch.full((R, H), float("nan"), device=DEV), torch.full((R, 3 * H), float("nan"), device=DEV),
                        torch.full((R, H), float("nan"), device=DEV))
        if new:
            hpi = h2i.HImage.from_tensor(hp)
            _ffi.check(lib.dtc_gru_h2i_image(c(W), p(img), H, 0, _ffi.stream()), "image")
            _ffi.check(lib.dtc_gru_step_fwd_h2i(hpi.ptr(), c(hp), p(img), c(b), c(gi), p(h), p(gates), p(hn), None, None, None, None, 0, None,
                                                None, R, H, _ffi.stream()), "step")
        else:
            _ffi.check(lib.dtc_gru_step_fwd(c(hp), c(W), c(b), c(gi), p(h), p(gates), p(hn), R, H, _ffi.stream()), "step")
        outs.append((h, gates, hn))
    gh = hp.double() @ W.double().T + b.double()
    r, z = torch.sigmoid(gi[:, :H].double() + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H].double() + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:].double() + r * gh[:, 2 * H:])
    ref = ((1 - z) * n + z * hp.double(), torch.cat([r, z, n], 1), gh[:, 2 * H:])
    for k in range(3):
        e32 = float((outs[0][k].double() - ref[k]).abs().max())
        enew = float((outs[1][k].double() - ref[k]).abs().max())
        print(f"gru step R={R} H={H} output {k}: fp32 MFMA err {e32:.2e}, image err {enew:.2e}")
        assert np.isfinite(enew) and enew <= 2.0 * e32 + 1e-6, (k, e32, enew)
    dgh = torch.randn(R, 3 * H, generator=g).to(DEV)
    ref = dgh.double() @ W.double()
    dghi = h2i.HImage.from_tensor(dgh)
    _ffi.check(lib.dtc_gru_h2i_image(c(W), p(img), H, 1, _ffi.stream()), "image")
    p32 = torch.full((3, R, H), float("nan"), device=DEV)
    _ffi.check(lib.dtc_linear_dgrad_split(c(dgh), 3 * H, c(W), p(p32), H, R * H, R, 3 * H, H, 3, _ffi.stream()), "split")
    e32 = float((p32.double().sum(0) - ref).abs().max() / ref.abs().max())
    for nparts in (1, 3, 6):
        part = torch.full((nparts, R, H), float("nan"), device=DEV)
        _ffi.check(lib.dtc_gru_dgrad_parts_h2i(dghi.ptr(), p(img), p(part), R * H, R, H, nparts, _ffi.stream()), "parts")
        enew = float((part.double().sum(0) - ref).abs().max() / ref.abs().max())
        print(f"gru dgrad chunks R={R} H={H} nparts={nparts}: fp32 MFMA err {e32:.2e}, image err {enew:.2e}")
        assert np.isfinite(enew) and enew <= 2.0 * e32 + 2e-7, (nparts, e32, enew)


def test_bad_arguments_are_refused():
    from dtc_amd import _ffi
    lib = _ffi.lib()
    assert lib.dtc_gru_h2i_workspace(24, 64, 192) == 0 and lib.dtc_gru_h2i_workspace(24, 64, 256) > 0
    t = torch.zeros(4096, device=DEV)
    a = _ffi.ptr(t)
    assert lib.dtc_gru_fwd_h2i(a, a, a, a, a, a, a, a, None, 0, None, None, 2, 4, 192, None) == -1
    assert lib.dtc_gru_fwd_h2i(a, None, a, a, a, a, a, a, None, 0, None, None, 2, 4, 128, None) == -1
    assert lib.dtc_gru_bwd_h2i(a, a, a, a, a, a, None, a, None, 0, None, None, None, None, None, 2, 4, 128, None) == -1
    assert lib.dtc_gru_h2i_image(a, a, 100, 0, None) == -1


@pytest.mark.parametrize("T,R,H", [(1, 64, 128), (2, 1, 128), (5, 7, 256), (24, 77, 512), (24, 1473, 512)])
def test_whole_recurrence_vs_fp64_and_the_default_path(T, R, H):
    from dtc_amd import ops
    x = _inputs(T, R, H, T * 1000 + R)
    new = _check_next_to_default(x, f"T={T} R={R} H={H}")
    again = _run(x, True)
    for k in FWD + BWD:
        assert torch.equal(new[k], again[k]), ("two runs differ", k)
    # rows are independent: the row-reversed problem gives the row-reversed outputs bit for bit
    xr = dict(x, gi=x["gi"].flip(1).contiguous(), h0=x["h0"].flip(0).contiguous(), dhs=x["dhs"].flip(1).contiguous())
    rev = _run(xr, True)
    for k in FWD + BWD:
        assert torch.equal(new[k], rev[k].flip(0 if k == "dh0" else 1)), ("row-reversed problem", k)


def test_heavy_tailed_gradients_keep_every_row_accurate():
    """dhs rows scaled by 10^u, u uniform in [-6, 6]: every row of dgi and dgh_all relative to that row's own largest element, next to the
    default path (test_hip_h2i.py's per-row bound)."""
    T, R, H = 6, 200, 256
    x = _inputs(T, R, H, 5)
    g = torch.Generator(device=DEV).manual_seed(6)
    x["dhs"] = torch.randn(T, R, H, device=DEV, generator=g) * 10.0 ** (12.0 * torch.rand(T, R, 1, device=DEV, generator=g) - 6.0)
    ref, new, old = _ref64(x), _run(x, True), _run(x, False)
    for k in ("dgi", "dgh"):
        den = ref[k].abs().amax(dim=2)
        live = den > 0
        en, eo = (float(((o[k].double() - ref[k]).abs().amax(dim=2)[live] / den[live]).max()) for o in (new, old))
        print(f"gru h2i heavy-tailed {k}: largest per-row relative error new {en:.3e}, default {eo:.3e}")
        assert np.isfinite(en) and en <= 2.0 * eo + 2e-6, (k, en, eo)


def _all_valid(T, R):
    return torch.arange(T * R, dtype=torch.int32, device=DEV)


def test_exponent_rule_and_containment():
    """Rows of h0 with a largest element of 30, all zero and 1e-3 hold the bounds of the whole-recurrence test; a NaN in one row of gi
    stays in that trajectory: every other row of every fp32 output and of every image is bit-identical to the clean run."""
    T, R, H = 5, 40, 256
    x = _inputs(T, R, H, 77)
    x["h0"][0] *= 30.0 / x["h0"][0].abs().max()
    x["h0"][1] = 0.0
    x["h0"][2] *= 1e-3 / x["h0"][2].abs().max()
    _check_next_to_default(x, "odd h0 rows")
    slot = _all_valid(T, R)
    clean = _run(x, True, slot, T * R, images=True)
    xn = dict(x, gi=x["gi"].clone())
    xn["gi"][1, 5, 7] = float("nan")
    dirty = _run(xn, True, slot, T * R, images=True)
    keep = torch.ones(R, dtype=torch.bool, device=DEV)
    keep[5] = False
    for k in FWD + BWD:
        a, b = (o[k] if k == "dh0" else o[k].transpose(0, 1) for o in (clean, dirty))
        assert torch.isfinite(a).all(), k
        assert torch.equal(a[keep], b[keep]), k
        assert not torch.isfinite(b[5]).all(), k
    keep_rows = keep.repeat(T)
    for k, im in clean["images"].items():
        a, b = im.to_tensor(), dirty["images"][k].to_tensor()
        assert torch.isfinite(a).all(), k
        assert torch.equal(a[keep_rows], b[keep_rows]), k
        ea, eb = (i.exps().permute(0, 2, 1).reshape(-1, i.exps().shape[1])[:T * R] for i in (im, dirty["images"][k]))
        assert torch.equal(ea[keep_rows], eb[keep_rows]), k


def test_valid_row_images():
    """With a slot map the kernels write the head's valid-row images themselves: each decodes to the gathered fp32 rows within twice the
    format's guarantee, rows behind M stay empty, and the fp32 outputs do not depend on the images being asked for."""
    T, R, H = 7, 50, 256
    x = _inputs(T, R, H, 9)
    g = torch.Generator(device=DEV).manual_seed(10)
    lens = torch.randint(1, T + 1, (R,), device=DEV, generator=g)
    lens[::7] = T
    valid = torch.arange(T, device=DEV)[:, None] < lens[None, :]                  # [T, R]
    x["dhs"] = x["dhs"] * valid[:, :, None]                                        # padded steps carry no gradient
    unpad_idx = valid.reshape(-1).nonzero().squeeze(1)                             # valid row -> padded slot, time-major
    M = unpad_idx.numel()
    assert M % 128 != 0 and M < T * R
    from dtc_amd import ops
    slot = ops.gru_slot_row(unpad_idx, T * R)
    assert slot.dtype == torch.int32 and int((slot >= 0).sum()) == M and torch.equal(slot[unpad_idx].long(), torch.arange(M, device=DEV))
    o = _run(x, True, slot, M, images=True)
    plain = _run(x, True)
    for k in FWD + BWD:
        assert torch.equal(o[k], plain[k]), k
    hs, dgh, dgi = o["hs"], o["dgh"].view(T * R, 3 * H), o["dgi"].view(T * R, 3 * H)
    want = dict(hx=hs[1:].reshape(T * R, H), hp=hs[:T].reshape(T * R, H), drz=dgh[:, :2 * H], dnh=dgh[:, 2 * H:], dni=dgi[:, 2 * H:], dgh=dgh, dgi=dgi)
    for k, im in o["images"].items():
        src = want[k][unpad_idx].double()
        got = im.to_tensor().double()
        blockmax = src.view(M, -1, 128).abs().amax(dim=2, keepdim=True)
        bound = torch.maximum(2.0 ** -21 * blockmax, torch.tensor(2.0 ** -37, device=DEV, dtype=torch.float64))
        err = (got - src).view(M, -1, 128).abs()
        print(f"gru h2i image {k}: largest error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), k
        ex = im.exps().permute(0, 2, 1).reshape(-1, im.exps().shape[1])
        assert bool((ex[M:] == 0x7fff).all()), (k, "rows behind M must stay empty")
        assert bool((ex[:M] != 0x7fff).any()), k
