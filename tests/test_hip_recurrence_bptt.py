"""The GRU and LSTM BPTT kernels (csrc/gru.hip, csrc/gru_s3.hip, csrc/lstm.hip, the fused steps and the split data gradient of
csrc/gemm.hip) against the float64 recurrences of tests/recurrence_ref.py: every output, per row, on every path the host drivers
choose between.  GPU only.

Every per-row output (hs_all[1:], cs_all[1:], gates, hn, dgi, dgh_all, dh0, dc0) is held to row_rel <= bound(e32): its error in a row
over that row's largest reference element, against 8 x the same figure of the reference's own fp32 run on the CPU (at least 2^-20,
at most 2e-5).  dW_hh / db_hh are held to the S measure of the product of the operands the kernels themselves left (dgh_all / dgi and
hs_all[:T], see recurrence_ref.measure).  No case needed a kernel fix.  The tables are one run on an MI355X, one line per case and
path; e32 is the figure of the CPU that ran next to it (the fp32 matrix products of another CPU's library sum in another order,
and e32 moves by up to a factor of two with it).

LSTM (dtc_lstm_fwd / dtc_lstm_fwd_fused, then dtc_lstm_bwd); every entry is error / e32 / bound in units of 1e-7:

path, (T, R, H), kind                                    hs               cs            gates              dgi              dh0              dc0               dW               db
lstm_fwd (1, 5, 32) plain                       1.0/1.0/9.5      0.9/1.0/9.5     1.6/1.5/12.3     1.5/1.5/12.1     2.3/3.6/29.1      2.7/1.1/9.5     1.4/1.7/13.3      1.1/0.6/9.5
lstm_fwd_fused (1, 5, 32) plain                 1.0/1.0/9.5      0.9/1.0/9.5     1.5/1.5/12.3     1.5/1.5/12.1     2.0/3.6/29.1      1.7/1.1/9.5     1.7/1.7/13.3      0.8/0.6/9.5
lstm_fwd (2, 1, 96) plain                      1.1/2.2/17.5      1.7/1.1/9.5     2.4/1.6/12.8     2.0/3.0/24.1     2.5/6.6/52.5      0.6/0.5/9.5      1.1/1.1/9.5      0.6/0.6/9.5
lstm_fwd_fused (2, 1, 96) plain                1.6/2.2/17.5      2.4/1.1/9.5     3.6/1.6/12.8     1.7/3.0/24.1     2.6/6.6/52.5      0.6/0.5/9.5      1.1/1.1/9.5      0.6/0.6/9.5
lstm_fwd (3, 5, 36) plain                      1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.7/1.8/14.7     2.9/3.1/24.5     2.1/2.9/23.1     3.3/1.5/12.0      0.8/0.7/9.5
lstm_fwd_fused (3, 5, 36) plain                1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.7/1.8/14.7     2.9/3.1/24.5     2.1/2.9/23.1     3.3/1.5/12.0      0.8/0.7/9.5
lstm_fwd (3, 5, 36) heavy                      1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.9/2.1/17.2     2.8/4.5/36.2     2.0/2.6/21.1     3.5/1.8/14.2     1.0/1.4/11.1
lstm_fwd_fused (3, 5, 36) heavy                1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.9/2.1/17.2     2.8/4.5/36.2     2.0/2.6/21.1     3.5/1.8/14.2     1.0/1.4/11.1
lstm_fwd (3, 5, 36) saturated                  1.4/1.4/11.3     1.7/2.1/16.9     1.4/1.4/11.6     4.2/4.2/33.5     3.3/4.8/38.0     1.5/1.4/11.3     2.3/1.4/11.6      1.5/0.9/9.5
lstm_fwd_fused (3, 5, 36) saturated            1.4/1.4/11.3     1.7/2.1/16.9     1.4/1.4/11.6     4.2/4.2/33.5     3.3/4.8/38.0     1.5/1.4/11.3     2.3/1.4/11.6      1.5/0.9/9.5
lstm_fwd (3, 5, 36) padded                     1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.7/1.8/14.6     2.1/2.9/23.2     2.0/2.9/23.1     2.7/1.5/11.8      0.9/0.7/9.5
lstm_fwd_fused (3, 5, 36) padded               1.5/1.6/12.4     1.7/1.7/13.3     1.9/1.4/11.6     2.7/1.8/14.6     2.1/2.9/23.2     2.0/2.9/23.1     2.7/1.5/11.8      0.9/0.7/9.5
lstm_fwd (3, 5, 37) plain                      1.9/1.8/14.3     1.5/1.5/12.2     1.8/1.4/11.1     1.8/2.1/16.6     1.7/3.6/29.1     1.4/1.4/11.1     2.2/1.3/10.2      1.1/0.8/9.5
lstm_fwd_fused (3, 5, 37) plain                1.9/1.8/14.3     1.5/1.5/12.2     1.8/1.4/11.1     1.8/2.1/16.6     1.7/3.6/29.1     1.4/1.4/11.1     2.2/1.3/10.2      1.1/0.8/9.5
lstm_fwd (5, 129, 64) plain                    2.8/3.3/26.4     3.2/3.1/24.5     4.1/3.6/29.0     4.6/3.9/31.6     4.9/6.1/48.4     3.7/2.9/23.0     1.2/1.8/14.3      0.2/0.2/9.5
lstm_fwd_fused (5, 129, 64) plain              2.7/3.3/26.4     3.1/3.1/24.5     3.5/3.6/29.0     3.7/3.9/31.6     4.8/6.1/48.4     2.9/2.9/23.0     1.4/1.8/14.3      0.2/0.2/9.5
lstm_fwd (6, 130, 128) plain                   4.0/4.0/31.9     3.4/3.4/26.9     6.0/4.8/38.2     4.7/3.9/31.5     6.1/5.8/46.8     3.2/3.1/25.2     1.3/1.4/11.3      0.2/0.2/9.5
lstm_fwd_fused (6, 130, 128) plain             4.7/4.0/31.9     3.4/3.4/26.9     4.8/4.8/38.2     4.9/3.9/31.5     6.1/5.8/46.8     3.9/3.1/25.2     1.1/1.4/11.3      0.2/0.2/9.5
lstm_fwd (6, 130, 128) heavy                   4.0/4.0/31.9     3.4/3.4/26.9     6.0/4.8/38.2     6.9/6.0/47.7     6.5/6.8/54.2     6.6/4.4/35.0     4.3/4.5/36.0      0.6/0.7/9.5
lstm_fwd_fused (6, 130, 128) heavy             4.7/4.0/31.9     3.4/3.4/26.9     4.8/4.8/38.2     5.9/6.0/47.7     5.7/6.8/54.2     4.7/4.4/35.0     4.1/4.5/36.0      0.5/0.7/9.5
lstm_fwd (6, 130, 128) saturated               3.6/4.5/36.4     3.2/3.7/29.9     5.1/5.7/45.6     5.8/5.8/46.0     5.5/6.2/49.6     3.3/3.7/29.5     2.0/1.8/14.4      0.4/0.3/9.5
lstm_fwd_fused (6, 130, 128) saturated         4.4/4.5/36.4     3.2/3.7/29.9     5.1/5.7/45.6     5.8/5.8/46.0     5.1/6.2/49.6     3.4/3.7/29.5     2.0/1.8/14.4      0.3/0.3/9.5
lstm_fwd (6, 130, 128) padded                  4.0/4.0/31.9     3.4/3.4/26.9     6.0/4.8/38.2     5.1/4.4/35.1     6.1/6.3/50.5     3.2/3.1/25.2     1.8/1.7/13.3      0.3/0.2/9.5
lstm_fwd_fused (6, 130, 128) padded            4.7/4.0/31.9     3.4/3.4/26.9     4.8/4.8/38.2     4.6/4.4/35.1     6.1/6.3/50.5     3.8/3.1/25.2     1.5/1.7/13.3      0.2/0.2/9.5
lstm_fwd (24, 13, 256) plain                   3.6/2.8/22.5     3.0/2.5/19.9     6.4/4.3/34.4     4.0/3.6/29.1     8.1/5.7/45.9     2.3/2.6/21.1     1.5/1.3/10.8      0.4/0.6/9.5
lstm_fwd_fused (24, 13, 256) plain             3.7/2.8/22.5     3.0/2.5/19.9     6.4/4.3/34.4     4.8/3.6/29.1     7.3/5.7/45.9     2.9/2.6/21.1     1.6/1.3/10.8      0.4/0.6/9.5

GRU (dtc_gru_fwd, dtc_gru_bwd; split = the split-precision switch; `rows` = with the valid slots), same units:

path, (T, R, H), kind                                    hs            gates               hn              dgi              dgh              dh0               dW               db
gru split=0 (1, 5, 32) plain                   1.3/1.3/10.0      0.8/0.8/9.5     2.5/2.5/19.8     2.2/1.7/13.8     1.6/1.6/12.9      1.6/1.1/9.5     1.2/1.3/10.1      1.0/1.0/9.5
gru split=1 (1, 5, 32) plain                   1.3/1.3/10.0      0.8/0.8/9.5     2.5/2.5/19.8     2.2/1.7/13.8     1.6/1.6/12.9      1.6/1.1/9.5     1.2/1.3/10.1      1.0/1.0/9.5
gru split=0 (2, 1, 96) plain                    1.0/0.9/9.5      1.1/1.1/9.5     2.2/1.6/12.5      1.7/1.2/9.7      1.5/1.1/9.5      1.2/1.2/9.8      1.1/1.1/9.5      0.6/0.6/9.5
gru split=1 (2, 1, 96) plain                    1.0/0.9/9.5      1.1/1.1/9.5     2.2/1.6/12.5      1.7/1.2/9.7      1.5/1.1/9.5      1.2/1.2/9.8      1.1/1.1/9.5      0.6/0.6/9.5
gru split=0 (3, 5, 36) plain                   1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     2.3/2.6/20.5     1.9/2.6/21.1     2.2/2.5/20.4     1.9/1.3/10.5      0.7/0.8/9.5
gru split=1 (3, 5, 36) plain                   1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     2.3/2.6/20.5     1.9/2.6/21.1     2.2/2.5/20.4     1.9/1.3/10.5      0.7/0.8/9.5
gru split=0 (3, 5, 36) heavy                   1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     2.2/1.6/13.1     2.7/2.1/16.8     1.9/1.8/14.2     2.3/1.4/11.1      1.3/1.1/9.5
gru split=1 (3, 5, 36) heavy                   1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     2.2/1.6/13.1     2.7/2.1/16.8     1.9/1.8/14.2     2.3/1.4/11.1      1.3/1.1/9.5
gru split=0 (3, 5, 36) saturated               1.8/1.8/14.4     1.3/1.9/15.1     1.9/2.5/19.6     6.2/6.2/49.7     6.2/6.2/49.7     1.7/2.3/18.5     1.9/1.4/11.1      0.9/0.8/9.5
gru split=1 (3, 5, 36) saturated               1.8/1.8/14.4     1.3/1.9/15.1     1.9/2.5/19.6     6.2/6.2/49.7     6.2/6.2/49.7     1.7/2.3/18.5     1.9/1.4/11.1      0.9/0.8/9.5
gru split=0 (3, 5, 36) padded                  1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     1.8/2.6/20.5     1.9/2.6/21.1     1.7/2.5/20.4     2.3/1.6/12.4      0.8/0.8/9.5
gru split=1 (3, 5, 36) padded                  1.7/1.6/13.0     2.6/1.9/15.1     2.6/2.5/19.6     1.8/2.6/20.5     1.9/2.6/21.1     1.7/2.5/20.4     2.3/1.6/12.4      0.8/0.8/9.5
gru split=0 (3, 5, 37) plain                   1.4/1.4/11.2     1.6/1.3/10.0     2.4/3.3/26.0     1.8/1.3/10.6     2.9/1.9/15.3     2.0/2.3/18.8      2.1/1.2/9.8      0.9/0.8/9.5
gru split=1 (3, 5, 37) plain                   1.4/1.4/11.2     1.6/1.3/10.0     2.4/3.3/26.0     1.8/1.3/10.6     2.9/1.9/15.3     2.0/2.3/18.8      2.1/1.2/9.8      0.9/0.8/9.5
gru split=0 (5, 129, 64) plain                 2.8/3.0/24.0     4.0/4.2/33.9     4.2/5.2/41.6     3.3/3.2/25.7     3.6/3.6/28.6     2.8/2.6/20.8      0.9/1.2/9.5      0.2/0.3/9.5
gru split=1 (5, 129, 64) plain                 2.8/3.0/24.0     4.0/4.2/33.9     4.2/5.2/41.6     3.3/3.2/25.7     3.6/3.6/28.6     2.8/2.6/20.8      0.9/1.2/9.5      0.2/0.3/9.5
gru split=0 (3, 130, 128) plain                3.5/3.3/26.1     4.6/4.7/37.5     6.9/5.7/45.9     4.0/3.6/28.6     3.7/4.3/34.1     2.7/3.5/27.8     1.2/1.8/14.4      0.5/0.3/9.5
gru split=1 (3, 130, 128) plain                3.5/3.3/26.1     4.6/4.7/37.5     6.9/5.7/45.9     4.0/3.6/28.6     3.8/4.3/34.1     3.1/3.5/27.8     1.5/1.8/14.4      0.4/0.3/9.5
gru split=0 (6, 130, 128) plain                5.6/5.9/47.2     6.0/6.1/48.8     6.8/6.2/49.6     4.2/4.2/33.3     4.5/4.5/35.8     3.2/4.2/33.3      0.9/1.0/9.5      0.2/0.3/9.5
gru split=1 (6, 130, 128) plain                3.1/5.9/47.2     5.0/6.1/48.8     5.8/6.2/49.6     3.9/4.2/33.3     3.9/4.5/35.8     3.9/4.2/33.3      0.9/1.0/9.5      0.2/0.3/9.5
gru split=0 (6, 130, 128) heavy                5.6/5.9/47.2     6.0/6.1/48.8     6.8/6.2/49.6     4.8/5.6/44.6     8.2/5.7/45.8     4.7/6.2/49.9     3.0/3.4/27.6      0.5/0.5/9.5
gru split=1 (6, 130, 128) heavy                3.1/5.9/47.2     5.0/6.1/48.8     5.8/6.2/49.6     5.9/5.6/44.6     6.0/5.7/45.8     4.3/6.2/49.9     2.9/3.4/27.6      0.6/0.5/9.5
gru split=0 (6, 130, 128) saturated            7.2/6.9/55.4     8.3/8.8/70.3     6.9/6.9/55.0     8.5/7.4/59.0     8.6/7.4/59.4     3.3/4.2/33.3     1.6/1.7/13.5      0.5/0.4/9.5
gru split=1 (6, 130, 128) saturated            4.5/6.9/55.4     5.2/8.8/70.3     5.8/6.9/55.0     6.7/7.4/59.0     7.2/7.4/59.4     3.9/4.2/33.3     1.7/1.7/13.5      0.4/0.4/9.5
gru split=0 (6, 130, 128) padded               5.6/5.9/47.2     6.0/6.1/48.8     6.8/6.2/49.6     4.2/3.9/31.4     4.5/4.5/35.8     3.0/4.2/33.3     1.3/1.5/11.9      0.2/0.3/9.5
gru split=1 (6, 130, 128) padded               3.1/5.9/47.2     5.0/6.1/48.8     5.8/6.2/49.6     3.8/3.9/31.4     4.0/4.5/35.8     3.4/4.2/33.3     1.0/1.5/11.9      0.3/0.3/9.5
gru split=0 (5, 40, 512) plain                 6.4/3.0/23.8     9.4/4.8/38.6    12.4/4.9/39.1     5.5/2.8/22.2     9.5/3.6/28.4     3.3/2.7/21.4     2.0/1.7/13.2      0.4/0.5/9.5
gru split=1 (5, 40, 512) plain                 7.2/3.0/23.8     9.6/4.8/38.6     8.5/4.9/39.1     4.7/2.8/22.2     5.1/3.6/28.4     4.0/2.7/21.4     1.7/1.7/13.2      0.5/0.5/9.5
gru split=1 rows (8, 200, 128) padded          4.6/3.9/31.3     5.2/5.6/45.1     7.4/7.9/63.4     3.6/4.3/34.6     4.9/5.1/40.6     4.4/3.7/29.5      0.6/0.7/9.5      0.3/0.2/9.5
gru split=1 (8, 200, 128) padded               4.6/3.9/31.3     5.2/5.6/45.1     7.4/7.9/63.4     3.6/4.3/34.6     4.9/5.1/40.6     4.4/3.7/29.5      0.8/0.7/9.5      0.3/0.2/9.5
gru split=0 (8, 200, 128) padded               4.2/3.9/31.3     4.9/5.6/45.1     7.0/7.9/63.4     3.8/4.3/34.6     5.1/5.1/40.6     3.6/3.7/29.5      0.6/0.7/9.5      0.2/0.2/9.5
"""
import contextlib

import pytest
import torch

import recurrence_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@contextlib.contextmanager
def _switches(split):
    """The per-step kernels (no persistent launch) with the split-precision switch at `split`; both restored."""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    prev = lib.dtc_get_gemm_split()
    lib.dtc_set_gru_seq(0)
    lib.dtc_set_gemm_split(int(split))
    try:
        yield lib
    finally:
        lib.dtc_set_gemm_split(prev)
        lib.dtc_set_gru_seq(-1)


@contextlib.contextmanager
def _profile():
    """-> a function that returns {kernel class: (launches, work)} since the last call (the library's own launch profile)"""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    lib.dtc_prof_enable(1)
    lib.dtc_prof_reset()

    def take():
        torch.cuda.synchronize()
        rep = {}
        for r in _ffi.prof_report():
            n, w = rep.get(r["name"].split("[")[0].strip(), (0, 0.0))
            rep[r["name"].split("[")[0].strip()] = (n + r["launches"], w + r["work"])
        lib.dtc_prof_reset()
        return rep
    try:
        yield take
    finally:
        lib.dtc_prof_enable(0)
        lib.dtc_prof_reset()


def _nan(*s):
    return torch.full(s, NAN, device=DEV)


def _workspace(nbytes, shift):
    """NaN-filled; shift: 8 bytes off the 16-byte boundary that torch's allocator gives"""
    from dtc_amd import ops
    ws = ops.workspace(nbytes + 8, DEV)[1:] if shift else ops.workspace(nbytes, DEV)
    assert ws.data_ptr() % 16 == (8 if shift else 0)
    ws.view(torch.float32).fill_(NAN)
    return ws


def _dev(x, *keys):
    return [x[k].to(DEV).contiguous() for k in keys]


def _run_gru(x, split, rows=None, shift=False, take=None):
    """dtc_gru_fwd + dtc_gru_bwd (with the W_hh weight gradient) -> every output by the reference's names; `take`: the launch profile of
    the forward and of the backward call lands in out["prof"]."""
    from dtc_amd import ops
    gi, h0, W, b, dhs = _dev(x, "gi", "h0", "W", "b", "dhs")
    T, R, H = dhs.shape
    with _switches(split):
        ws = _workspace(ops.gru_workspace_bytes(T, R, H), shift)               # (sized behind the switch: the layout depends on it)
        o = dict(hs=_nan(T + 1, R, H), gates=_nan(T, R, 3 * H), hn=_nan(T, R, H), dgi=_nan(T, R, 3 * H), dh0=_nan(R, H),
                 dW=_nan(3 * H, H), db=_nan(3 * H))
        prof = []
        if take:
            take()
        ops.gru_fwd(gi, h0, W, b, o["hs"], o["gates"], o["hn"], ws)
        if take:
            prof.append(take())
        ops.gru_bwd(dhs, o["hs"], o["gates"], o["hn"], W, o["dgi"], o["dW"], o["db"], o["dh0"], ws, rows=rows)
        if take:
            prof.append(take())
        torch.cuda.synchronize()
        o["dgh"] = ops.gru_dgh_all(ws, T, R, H).view(T, R, 3 * H).clone()
    assert torch.equal(o["hs"][0], h0)
    if take:
        o["prof"] = prof
    return o


def _run_lstm(x, fwd, shift=False):
    """dtc_lstm_fwd or dtc_lstm_fwd_fused, then dtc_lstm_bwd from its saved tensors"""
    from dtc_amd import ops
    gi, h0, c0, W, b, dhs = _dev(x, "gi", "h0", "c0", "W", "b", "dhs")
    T, R, H = dhs.shape
    with _switches(0):
        ws = _workspace(ops.lstm_workspace_bytes(T, R, H), shift)
        o = dict(hs=_nan(T + 1, R, H), cs=_nan(T + 1, R, H), gates=_nan(T, R, 4 * H), dgi=_nan(T, R, 4 * H), dh0=_nan(R, H), dc0=_nan(R, H),
                 dW=_nan(4 * H, H), db=_nan(4 * H))
        getattr(ops, fwd)(gi, h0, c0, W, b, o["hs"], o["cs"], o["gates"], ws)
        ops.lstm_bwd(dhs, o["hs"], o["cs"], o["gates"], W, o["dgi"], o["dW"], o["db"], o["dh0"], o["dc0"], ws)
        torch.cuda.synchronize()
    assert torch.equal(o["hs"][0], h0) and torch.equal(o["cs"][0], c0)
    return o


def _tensors(o):
    return {k: v for k, v in o.items() if isinstance(v, torch.Tensor)}


def _hold(cell, what, o, x, ref, e32):
    """every quantity finite and within bound(e32) of fp64; for `padded`, the dead rows of dgi / dgh exactly zero"""
    o = _tensors(o)
    for k, v in o.items():
        assert bool(torch.isfinite(v).all()), (what, k, "a slot nobody wrote, or a non-finite result")
    err, _ = rr.measure(cell, o, ref)
    bad = []
    for k in err:
        bd = rr.bound(e32[k])
        print(f"BPTT {what} | {k} | err {err[k]:.3e} | e32 {e32[k]:.3e} | bound {bd:.3e}")
        if not err[k] <= bd:
            bad.append((k, err[k], e32[k], bd))
    assert not bad, (what, bad)
    if "rows" in x:
        T, R = x["dhs"].shape[:2]
        dead = torch.ones(T * R, dtype=torch.bool)
        dead[x["rows"]] = False
        for k in ("dgi", "dgh"):
            if k in o:
                assert float(o[k].reshape(T * R, -1).cpu()[dead].abs().max()) == 0.0, (what, k, "dead rows")


# ---------------------------------------------------------------- A. LSTM, all outputs
@pytest.mark.parametrize("fwd", ["lstm_fwd", "lstm_fwd_fused"])
@pytest.mark.parametrize("T,R,H,kind", rr.LSTM_CASES)
def test_lstm_every_output_vs_fp64(T, R, H, kind, fwd):
    x, ref, e32, _ = rr.case("lstm", T, R, H, kind)
    _hold("lstm", f"{fwd} ({T}, {R}, {H}) {kind}", _run_lstm(x, fwd), x, ref, e32)


# ---------------------------------------------------------------- B. GRU default paths
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("T,R,H,kind", rr.GRU_CASES)
def test_gru_every_output_vs_fp64_on_the_intended_path(T, R, H, kind, split):
    x, ref, e32, _ = rr.case("gru", T, R, H, kind)
    with _profile() as take:
        o = _run_gru(x, split, take=take)
    fwd, bwd = o["prof"]
    want_fwd, want_bwd_split = rr.gru_paths((T, R, H), split)
    launches = lambda p, k: p.get(k, (0, 0.0))[0]
    print(f"BPTT gru ({T}, {R}, {H}) split={split}: forward {fwd}, backward {bwd}")
    assert launches(fwd, "gru_gate_fwd") == (T if want_fwd == "unfused" else 0), fwd
    assert launches(fwd, "wimage") == (1 if want_fwd == "split" else 0), fwd
    assert launches(fwd, "gru_step_fwd") == (0 if want_fwd == "unfused" else T) and launches(fwd, "linear_fwd") == (T if want_fwd == "unfused" else 0), fwd
    assert launches(bwd, "wimage") == (1 if want_bwd_split else 0), bwd
    assert launches(bwd, "gru_gate_bwd") == T and launches(bwd, "linear_dgrad") == T and launches(bwd, "linear_wgrad") == 1, bwd
    _hold("gru", f"gru split={split} ({T}, {R}, {H}) {kind}", o, x, ref, e32)


# ---------------------------------------------------------------- C. valid_rows
OUT_GRU = ("hs", "gates", "hn", "dgi", "dgh", "dh0", "dW", "db")
OUT_LSTM = ("hs", "cs", "gates", "dgi", "dh0", "dc0", "dW", "db")


def _wgrad_work(o):
    return o["prof"][1]["linear_wgrad"][1]


def test_gru_valid_rows_route_vs_fp64_and_the_call_without_rows():
    """padded (8, 200, 128), 1138 valid slots of 1600: with the split switch on, dtc_gru_bwd hands the W_hh weight gradient to
    dtc_linear_wgrad_rows -- the profile counts its work on n_valid rows --, dW_hh / db_hh hold the S bound and nothing else changes;
    with the switch off, `rows` changes nothing."""
    T, R, H, kind = rr.VALID_ROWS_CASES[0]
    x, ref, e32, _ = rr.case("gru", T, R, H, kind)
    rows = x["rows"].to(DEV)
    n = rows.numel()
    assert 1024 <= n < T * R
    with _profile() as take:
        on, on_rows = _run_gru(x, 1, take=take), _run_gru(x, 1, rows=rows, take=take)
        off, off_rows = _run_gru(x, 0, take=take), _run_gru(x, 0, rows=rows, take=take)
    full, part = 2.0 * T * R * 3 * H * H, 2.0 * n * 3 * H * H
    assert (_wgrad_work(on), _wgrad_work(on_rows), _wgrad_work(off), _wgrad_work(off_rows)) == (full, part, full, full)
    _hold("gru", f"gru split=1 rows ({T}, {R}, {H}) {kind}", on_rows, x, ref, e32)
    _hold("gru", f"gru split=1 ({T}, {R}, {H}) {kind}", on, x, ref, e32)
    _hold("gru", f"gru split=0 ({T}, {R}, {H}) {kind}", off, x, ref, e32)
    for k in OUT_GRU[:-2]:
        assert torch.equal(on[k], on_rows[k]), k
    for k in OUT_GRU:
        assert torch.equal(off[k], off_rows[k]), k


@pytest.mark.parametrize("split", [0, 1])
def test_gru_valid_rows_below_the_threshold_change_nothing(split):
    T, R, H, kind = rr.VALID_ROWS_CASES[1]
    x = rr.case("gru", T, R, H, kind)[0]
    rows = x["rows"].to(DEV)
    assert rows.numel() < 1024
    with _profile() as take:
        a, b = _run_gru(x, split, take=take), _run_gru(x, split, rows=rows, take=take)
    assert _wgrad_work(a) == _wgrad_work(b) == 2.0 * T * R * 3 * H * H
    for k in OUT_GRU:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- D, E: one runner per entry point
RUNNERS = {
    "gru split=0": ("gru", OUT_GRU, lambda x, **kw: _run_gru(x, 0, **kw)),
    "gru split=1": ("gru", OUT_GRU, lambda x, **kw: _run_gru(x, 1, **kw)),
    "lstm_fwd": ("lstm", OUT_LSTM, lambda x, **kw: _run_lstm(x, "lstm_fwd", **kw)),
    "lstm_fwd_fused": ("lstm", OUT_LSTM, lambda x, **kw: _run_lstm(x, "lstm_fwd_fused", **kw)),
}


@pytest.mark.parametrize("T,R,H", rr.INVARIANT_SHAPES)
@pytest.mark.parametrize("which", list(RUNNERS))
def test_workspace_eight_bytes_off_a_16_byte_boundary(which, T, R, H):
    """ops.workspace promises 8-byte alignment; torch's allocator never gives less than 16.  The layouts place their aligned sub-buffers
    by address and the gate arithmetic is the same cell on the vector and the scalar kernels: every output has the same bits."""
    cell, keys, run = RUNNERS[which]
    x = rr.case(cell, T, R, H, "plain")[0]
    a, b = run(x), run(x, shift=True)
    for k in keys:
        assert bool(torch.isfinite(b[k]).all()), k
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("T,R,H", rr.INVARIANT_SHAPES)
@pytest.mark.parametrize("which", list(RUNNERS))
def test_two_runs_row_reversal_and_a_nan_row(which, T, R, H):
    cell, keys, run = RUNNERS[which]
    x = rr.case(cell, T, R, H, "plain")[0]
    clean, again = run(x), run(x)
    for k in keys:
        assert torch.equal(clean[k], again[k]), ("two runs differ", k)
    per_row = keys[:-2]
    rdim = lambda k: 0 if k in ("dh0", "dc0") else 1
    # rows are independent: the row-reversed problem gives the row-reversed outputs
    xr = {k: (v.flip(0 if k in ("h0", "c0") else 1).contiguous() if k in ("gi", "h0", "c0", "dhs") else v) for k, v in x.items()}
    rev = run(xr)
    for k in per_row:
        assert torch.equal(clean[k], rev[k].flip(rdim(k))), ("row-reversed problem", k)
    # a NaN stays in its trajectory
    r0 = R // 2
    xn = dict(x, gi=x["gi"].clone())
    xn["gi"][1, r0, 7] = NAN
    dirty = run(xn)
    keep = torch.ones(R, dtype=torch.bool, device=DEV)
    keep[r0] = False
    for k in per_row:
        a, b = (o[k].movedim(rdim(k), 0) for o in (clean, dirty))
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a[keep], b[keep]), ("a NaN in one row reached another", k)
        assert not bool(torch.isfinite(b[r0]).all()), k
    assert not bool(torch.isfinite(dirty["hs"][2:, r0]).all(-1).any()), "row r0 is non-finite from t = 1 on"
    assert bool(torch.isfinite(dirty["hs"][:2, r0]).all())
