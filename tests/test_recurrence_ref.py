"""tests/recurrence_ref.py on the CPU: its fp64 recurrences are torch.nn.GRU's / torch.nn.LSTM's, and on every case of the tables
that tests/test_hip_recurrence_bptt.py runs, the fp32 run of the same code -- the yardstick e32 of the kernels' bounds -- lies so
close to fp64 that the bounds' ceiling never decides a case, and the `padded` kind has the dead rows it is meant to have."""
import pytest
import torch

import recurrence_ref as rr

ALL_CASES = ([("lstm",) + c for c in rr.LSTM_CASES] + [("gru",) + c for c in rr.GRU_CASES] +
             [("gru",) + c for c in rr.VALID_ROWS_CASES if c not in rr.GRU_CASES])


def _close(a, b, what):
    a, b = a.detach(), b.detach()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert scale > 0 and err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("cell,T,R,H", [("gru", 3, 5, 36), ("gru", 6, 17, 64), ("lstm", 3, 5, 36), ("lstm", 6, 17, 64)])
def test_fp64_helper_is_torch_nn_in_double(cell, T, R, H):
    """torch.nn.GRU / LSTM in .double() with an identity input projection (x W_ih^T + b_ih = x exactly: the helper's gi) and autograd:
    outputs, final states, the input gradient and every parameter gradient."""
    G = 3 if cell == "gru" else 4
    x = rr.inputs(cell, T, R, H, rr.seed_of(T, R))
    ref = rr.REF[cell](x, torch.float64)
    rnn = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(input_size=G * H, hidden_size=H, num_layers=1).double()
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.eye(G * H, dtype=torch.float64))
        rnn.bias_ih_l0.zero_()
        rnn.weight_hh_l0.copy_(x["W"].double())
        rnn.bias_hh_l0.copy_(x["b"].double())
    xin = x["gi"].double().requires_grad_(True)
    h0 = x["h0"].double()[None].requires_grad_(True)
    if cell == "gru":
        out, hT = rnn(xin, h0)
    else:
        c0 = x["c0"].double()[None].requires_grad_(True)
        out, (hT, cT) = rnn(xin, (h0, c0))
        _close(cT[0], ref["cs"][-1], "c_T")
    (out * x["dhs"].double()).sum().backward()
    _close(out, ref["hs"][1:], "outputs")
    _close(hT[0], ref["hs"][-1], "h_T")
    assert torch.equal(ref["hs"][0], x["h0"].double())
    _close(xin.grad, ref["dgi"], "dgi")
    _close(h0.grad[0], ref["dh0"], "dh0")
    if cell == "lstm":
        _close(c0.grad[0], ref["dc0"], "dc0")
    _close(rnn.weight_hh_l0.grad, ref["dW"], "dW_hh")
    _close(rnn.bias_hh_l0.grad, ref["db"], "db_hh")
    dgi = ref["dgi"].reshape(T * R, G * H)
    _close(rnn.weight_ih_l0.grad, dgi.T @ x["gi"].double().reshape(T * R, G * H), "dW_ih")
    _close(rnn.bias_ih_l0.grad, dgi.sum(0), "db_ih")
    if cell == "gru":               # dgh differs from dgi in the n gate alone, by the factor r; hn is gh_n = atanh(n) - gi_n over r
        _close(ref["dgh"][..., :2 * H], ref["dgi"][..., :2 * H], "dgh r, z")
        _close(ref["dgh"][..., 2 * H:], ref["dgi"][..., 2 * H:] * ref["gates"][..., :H], "dgh n")
        _close(rnn.weight_hh_l0.grad, ref["dgh"].reshape(T * R, 3 * H).T @ ref["hs"][:-1].reshape(T * R, H), "dgh^T h")


def test_case_tables_are_the_ones_stated():
    assert len(rr.LSTM_CASES) == 7 + 6 and len(rr.GRU_CASES) == 8 + 6
    assert all(s in rr.LSTM_SHAPES and s in rr.GRU_SHAPES for s in rr.ALL_KINDS_SHAPES + rr.INVARIANT_SHAPES)
    for (T, R, H), (fwd, bwd) in rr.GRU_SHAPES.items():
        assert fwd == ("unfused" if H % 32 else "split" if H % 128 == 0 and T >= 4 else "fused") and bwd == (H % 128 == 0), (T, R, H)
        assert rr.gru_paths((T, R, H), 0) == ("unfused" if H % 32 else "fused", False)


@pytest.mark.parametrize("cell,T,R,H,kind", ALL_CASES)
def test_fp32_reference_run_is_far_below_the_ceiling(cell, T, R, H, kind):
    x, ref, e32, zero = rr.case(cell, T, R, H, kind)
    print(f"{cell} ({T}, {R}, {H}) {kind}: e32 " + " ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    for k, v in e32.items():
        assert v <= rr.CEILING / rr.MARGIN, (k, v)
        assert rr.bound(v) < rr.CEILING
    dead = T * R - x["rows"].numel() if kind == "padded" else 0
    for k, n in zero.items():
        assert n == (dead if k in ("dgi", "dgh") else 0), (k, n, dead)
    if kind == "padded":
        t, r = x["rows"] // R, x["rows"] % R
        assert bool((t < x["lens"][r]).all()) and x["rows"].numel() == int(x["lens"].sum()) and bool((x["rows"][1:] > x["rows"][:-1]).all())
        assert bool((x["lens"][::3] == T).all()) and 0 < dead
        assert bool((ref["dgi"].reshape(T * R, -1)[x["rows"]].abs().amax(1) > 0).all())


def test_valid_row_cases_sit_on_both_sides_of_the_threshold():
    (T, R, H, kind), (t, r, h, k) = rr.VALID_ROWS_CASES
    n = rr.inputs("gru", T, R, H, rr.seed_of(T, R), kind)["rows"].numel()
    assert (n, T * R) == (1138, 1600) and 1024 <= n < T * R and 3 * H * H >= 128 * 128
    m = rr.inputs("gru", t, r, h, rr.seed_of(t, r), k)["rows"].numel()
    assert (m, t * r) == (605, 780) and m < 1024
