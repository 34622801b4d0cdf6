"""float64 references, inputs, measures and case tables for the GRU / LSTM recurrence kernels (csrc/gru.hip, csrc/gru_s3.hip,
csrc/lstm.hip and the fused steps of csrc/gemm.hip).  A helper, not a test: tests/test_recurrence_ref.py checks it on the CPU,
tests/test_hip_recurrence_bptt.py holds the kernels to it.

The references are torch.nn.GRU's / torch.nn.LSTM's recurrence -- the modules the reference's `Memory` wraps
(actor_critic_recurrent.py:92-116) -- written out step by step on the pre-computed input projection gi = x W_ih^T + b_ih, with
the gradients of (hs[1:] * dhs).sum() by autograd.  They run in the dtype asked for: float64 is the truth, the float32 run of
the SAME code on the CPU is the yardstick `e32` that `bound` turns into what a kernel may miss the truth by."""
import functools

import torch

KINDS = ("plain", "heavy", "saturated", "padded")

# ---------------------------------------------------------------- case tables (T, R, H), shared by the CPU and the GPU test
# LSTM: (1, 5, 32) T = 1 (no chunks to add in the first gate kernel, dh0 summed straight away) and H = 32 (the fused step's K loop
# body never runs); (2, 1, 96) one row, three K iterations; (3, 5, 36) / (3, 5, 37) the GEMM + gate-kernel pair, rows on / off a
# 16-byte boundary; (5, 129, 64) a row tile with a one-row tail
LSTM_SHAPES = [(1, 5, 32), (2, 1, 96), (3, 5, 36), (3, 5, 37), (5, 129, 64), (6, 130, 128), (24, 13, 256)]
# GRU with the split switch ON: shape -> (forward step, split-precision backward).  "fused": dtc_gru_step_fwd (fp32 MFMA),
# "unfused": dtc_linear_fwd + gru_gate_fwd_kernel (H % 32 != 0), "split": csrc/gru_s3.hip (H % 128 == 0 and T >= 4).  With the
# switch OFF nothing runs on the split-precision path and the forward step depends on H % 32 alone.
GRU_SHAPES = {
    (1, 5, 32): ("fused", False),
    (2, 1, 96): ("fused", False),
    (3, 5, 36): ("unfused", False),          # four units per thread in the gate backward
    (3, 5, 37): ("unfused", False),          # one unit per thread
    (5, 129, 64): ("fused", False),
    (3, 130, 128): ("fused", True),          # T < 4: the fp32 step although the split path serves H
    (6, 130, 128): ("split", True),
    (5, 40, 512): ("split", True),           # four column tiles, six chunks of the data gradient
}
ALL_KINDS_SHAPES = [(3, 5, 36), (6, 130, 128)]          # these run every kind; the others run "plain"
VALID_ROWS_SHAPE = (8, 200, 128)                        # padded: 1024 <= n_valid < T * R (the dtc_linear_wgrad_rows route)
INVARIANT_SHAPES = [(3, 5, 36), (6, 130, 128)]


def cases(shapes):
    return [(T, R, H, k) for (T, R, H) in shapes for k in (KINDS if (T, R, H) in ALL_KINDS_SHAPES else KINDS[:1])]


LSTM_CASES = cases(LSTM_SHAPES)
GRU_CASES = cases(list(GRU_SHAPES))
VALID_ROWS_CASES = [VALID_ROWS_SHAPE + ("padded",), (6, 130, 128, "padded")]


def gru_paths(shape, split):
    """-> (forward step, split-precision backward) that dtc_gru_fwd / dtc_gru_bwd take for `shape` with the split switch at `split`."""
    fwd, bwd = GRU_SHAPES[shape]
    if not split:
        return ("fused" if shape[2] % 32 == 0 else "unfused"), False
    return fwd, bwd


# ---------------------------------------------------------------- inputs
def lengths(T, R):
    """trajectory length of every row of the `padded` kind"""
    r = torch.arange(R)
    return torch.where(r % 3 == 0, torch.full((R,), T), 1 + (7 * r) % T)


def inputs(cell, T, R, H, seed, kind="plain"):
    """fp32 CPU tensors gi [T, R, G H], h0 (c0) [R, H], W [G H, H], b [G H], dhs [T, R, H] (G = 3 for "gru", 4 for "lstm") from a CPU
    generator; `padded` adds lens [R] and rows = the sorted valid slots t * R + r (int64)."""
    assert cell in ("gru", "lstm") and kind in KINDS
    G = 3 if cell == "gru" else 4
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = dict(gi=rn(T, R, G * H), h0=0.5 * rn(R, H))
    if cell == "lstm":
        x["c0"] = 0.5 * rn(R, H)
    x.update(W=rn(G * H, H) / H ** 0.5, b=0.2 * rn(G * H), dhs=0.01 * rn(T, R, H))
    if kind == "heavy":
        x["dhs"] = rn(T, R, H) * 10.0 ** (12.0 * torch.rand(T, R, 1, generator=g) - 6.0)
    elif kind == "saturated":
        x["gi"][:, torch.arange(R) % 2 == 0] *= 8.0
        if cell == "lstm":
            x["c0"] *= 4.0
    elif kind == "padded":
        x["lens"] = lengths(T, R)
        valid = torch.arange(T)[:, None] < x["lens"][None, :]                  # [T, R]
        x["dhs"] = x["dhs"] * valid[:, :, None]
        x["rows"] = valid.reshape(-1).nonzero().squeeze(1)
    return x


def seed_of(T, R):
    return T * 1000 + R


# ---------------------------------------------------------------- references
def _leaves(x, keys, dtype, device):
    return {k: x[k].to(device=device, dtype=dtype).requires_grad_(True) for k in keys}


def gru_ref(x, dtype, device="cpu"):
    """gate order r, z, n; gh = h W^T + b; n = tanh(gi_n + r * gh_n); h = (1 - z) * n + z * h.
    -> hs [T + 1, R, H], gates [T, R, 3H], hn [T, R, H] (= gh_n), dgi, dgh [T, R, 3H], dh0, dW, db"""
    p = _leaves(x, ("gi", "h0", "W", "b"), dtype, device)
    dhs = x["dhs"].to(device=device, dtype=dtype)
    T, R, H3 = p["gi"].shape
    H = H3 // 3
    h, hs, gates, hn, ghs = p["h0"], [p["h0"]], [], [], []
    for t in range(T):
        gh = h @ p["W"].T + p["b"]
        gh.retain_grad()
        gi = p["gi"][t]
        r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h)
        gates.append(torch.cat([r, z, n], 1))
        hn.append(gh[:, 2 * H:])
        ghs.append(gh)
    (torch.stack(hs[1:]) * dhs).sum().backward()
    return dict(hs=torch.stack(hs).detach(), gates=torch.stack(gates).detach(), hn=torch.stack(hn).detach(), dgi=p["gi"].grad,
                dgh=torch.stack([g.grad for g in ghs]), dh0=p["h0"].grad, dW=p["W"].grad, db=p["b"].grad)


def lstm_ref(x, dtype, device="cpu"):
    """gate order i, f, g, o; a = gi + h W^T + b; c = f * c + i * g; h = o * tanh(c).
    -> hs, cs [T + 1, R, H], gates, dgi [T, R, 4H] (the gradient w.r.t. gi is the one w.r.t. gh), dh0, dc0, dW, db"""
    p = _leaves(x, ("gi", "h0", "c0", "W", "b"), dtype, device)
    dhs = x["dhs"].to(device=device, dtype=dtype)
    T, R, H4 = p["gi"].shape
    H = H4 // 4
    h, c, hs, cs, gates = p["h0"], p["c0"], [p["h0"]], [p["c0"]], []
    for t in range(T):
        a = p["gi"][t] + (h @ p["W"].T + p["b"])
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        gg = torch.tanh(a[:, 2 * H:3 * H])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gates.append(torch.cat([i, f, gg, o], 1))
    (torch.stack(hs[1:]) * dhs).sum().backward()
    return dict(hs=torch.stack(hs).detach(), cs=torch.stack(cs).detach(), gates=torch.stack(gates).detach(), dgi=p["gi"].grad,
                dh0=p["h0"].grad, dc0=p["c0"].grad, dW=p["W"].grad, db=p["b"].grad)


REF = dict(gru=gru_ref, lstm=lstm_ref)
# the per-row quantities of each cell (dW, db: the S measure)
ROW_KEYS = dict(gru=("hs", "gates", "hn", "dgi", "dgh", "dh0"), lstm=("hs", "cs", "gates", "dgi", "dh0", "dc0"))


# ---------------------------------------------------------------- measures
def _d(t):
    return t.detach().double().cpu()


def row_rel(got, ref):
    """-> (largest over the rows (all leading axes) of max|got - ref| / max|ref| along the last axis, over rows whose reference is
    non-zero; number of all-zero reference rows).  A non-finite `got` gives a non-finite measure."""
    got, ref = _d(got), _d(ref)
    num, den = (got - ref).abs().amax(-1), ref.abs().amax(-1)
    live = den > 0
    q = num[live] / den[live]
    err = float("nan") if bool(torch.isnan(q).any()) else float(q.max()) if q.numel() else 0.0
    return err, int((~live).sum())


def _over(err, S):
    if not bool(torch.isfinite(err).all() and torch.isfinite(S).all()):
        return float("nan")
    return float((err[S > 0] / S[S > 0]).max())


def s_rel(dW, ref, dZ, X):
    """max |dW - ref| / (|dZ|^T |X|) in fp64: the error of a weight gradient dZ^T X against the sum of the magnitudes of its terms
    (tests/test_hip_wgrad_image.py's normalisation); dZ [M, N], X [M, K]."""
    dW, ref, dZ, X = _d(dW), _d(ref), _d(dZ), _d(X)
    return _over((dW - ref).abs(), dZ.abs().T @ X.abs())


def s_rel_bias(db, ref, dZ):
    """max |db - ref| / colsum|dZ|"""
    db, ref, dZ = _d(db), _d(ref), _d(dZ)
    return _over((db - ref).abs(), dZ.abs().sum(0))


def s_rel_terms(got, ref, S):
    """max |got - ref| / S over the elements with S > 0, for a caller-supplied S of got's shape: the sum of the magnitudes of every
    element's own terms (a dense layer's |X| |W|^T + |b|), so a small element is judged against what it was added up from."""
    return _over((_d(got) - _d(ref)).abs(), _d(S))


def measure(cell, got, ref):
    """every quantity of `got` (a dict shaped like the reference's) against the fp64 reference `ref`
    -> ({quantity: error}, {quantity: all-zero reference rows}).  hs / cs are measured behind the initial state.

    dW / db are measured as tests/test_hip_wgrad_image.py measures a weight gradient: against the fp64 product of the operands the
    computation itself consumed -- got's own dgh (LSTM: dgi) and hs[:T] --, over the S of those operands.  The operands are held to
    fp64 by their row measures; what is left is the error of the product.  Measured against the autograd dW of the fp64 run instead,
    the S measure inherits the per-ELEMENT relative error of dgh (an element that cancels to 1e-3 of its row's largest carries a
    1e-4 relative error in fp32), and with the few rows of the small cases nothing averages it out: the fp32 reference run itself
    then reaches 7.3e-5 at gru (2, 1, 96), 8.4e-6 at lstm (2, 1, 96), 7.1e-6 / 3.3e-6 at lstm / gru (3, 5, 36) saturated -- as
    ill-conditioned as a per-feature row measure of dW_hh (9.8e-5 at saturated (1, 5, 64)), and as little use as a bound."""
    err, zero = {}, {}
    for k in ROW_KEYS[cell]:
        a, b = (got[k][1:], ref[k][1:]) if k in ("hs", "cs") else (got[k], ref[k])
        err[k], zero[k] = row_rel(a, b)
    dZ = _d(got["dgh" if cell == "gru" else "dgi"])
    dZ = dZ.reshape(-1, dZ.shape[-1])
    X = _d(got["hs"][:-1]).reshape(dZ.shape[0], -1)
    err["dW"] = s_rel(got["dW"], dZ.T @ X, dZ, X)
    err["db"] = s_rel_bias(got["db"], dZ.sum(0), dZ)
    return err, zero


FLOOR, CEILING, MARGIN = 2.0 ** -20, 2e-5, 8.0


def bound(e32):
    """What a kernel may miss fp64 by, in the measure in which the fp32 reference run misses it by e32: 8 x e32 (the margin the project
    gives a kernel over an fp32 computation of the same quantity: summation order of the MFMA products, expf / tanhf a few ulp off
    libm), at least 2^-20 (sixteen half-ulp roundings; the cells' backward expressions chain 8-10), at most 2e-5 (ROW_TOL of
    tests/test_gru_path.py)."""
    return min(CEILING, max(MARGIN * e32, FLOOR))


@functools.lru_cache(maxsize=None)
def case(cell, T, R, H, kind):
    """-> (inputs, fp64 reference, e32 per quantity, all-zero reference rows per quantity), computed once per case on the CPU; callers
    leave all of it unchanged"""
    x = inputs(cell, T, R, H, seed_of(T, R), kind)
    ref = REF[cell](x, torch.float64)
    e32, zero = measure(cell, REF[cell](x, torch.float32), ref)
    return x, ref, e32, zero
