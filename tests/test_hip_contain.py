"""Kernels of PPO(contain_nonfinite=True) (csrc/contain.hip, the contained forms in csrc/gae.hip) against numpy: the per-row validity
record (ops.rows_finite), the contained GAE scan and advantage statistics (rollout_storage.py:138-152 over the valid rows), the
compaction into the ascending list of valid rows and the permutation repair (rollout_storage.py:165 over valid rows).  References are
float64 / integer numpy written here; `ops.gae` is the bit-exact reference of the scan on valid rows (itself pinned to oracle/gae.py
by tests/test_hip_kernels.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda:0"
WIDTHS = (1, 3, 12, 53, 265, 1389)       # the row widths of the stored rollout tensors
R = 300


def _matrices():
    rng = np.random.default_rng(17)
    ms = [rng.standard_normal((R, w)).astype(np.float32) for w in WIDTHS]
    nan, inf = np.float32("nan"), np.float32("inf")
    ms[0][0, 0] = nan                    # first row, first (= last) column
    ms[1][0, 2] = inf                    # first row, last column
    ms[2][R - 1, 0] = -inf               # last row, first column
    ms[3][R - 1, 52] = nan               # last row, last column
    ms[4][150, 100] = inf                # interior
    ms[5][77, 1388] = -inf
    ms[5][200, 0] = nan
    ms[5][201, 694] = nan                # a 16-byte group in the middle of a row of 1389
    # finite: a denormal, -0.0, +-FLT_MAX
    ms[3][10, 5] = np.float32(1e-45)
    ms[4][11, 0] = np.float32(-0.0)
    ms[5][12, 7] = np.float32(3.4028235e38)
    ms[1][13, 1] = np.float32(-3.4028235e38)
    ms[0][14, 0] = np.float32(1.1754942e-38)     # the largest denormal
    return ms


def _want(ms):
    ok = np.ones(R, dtype=bool)
    for m in ms:
        ok &= np.isfinite(m).all(1)
    return ok


@pytest.mark.gpu
def test_row_scan_matches_numpy_at_every_width():
    from dtc_amd import ops
    ms = _matrices()
    want = _want(ms)
    assert want[[10, 11, 12, 13, 14]].all() and not want[[0, R - 1, 150, 77, 200, 201]].any() and int((~want).sum()) == 6
    ts = [torch.from_numpy(m).to(DEV) for m in ms]
    got = ops.rows_finite(ts)
    assert got.dtype == torch.uint8 and got.shape == (R,)
    assert np.array_equal(got.cpu().numpy().astype(bool), want)
    # one matrix at a time: each plant is found in the matrix it sits in
    for m, t in zip(ms, ts):
        assert np.array_equal(ops.rows_finite([t]).cpu().numpy().astype(bool), np.isfinite(m).all(1)), m.shape
    # a 0 already in `out` survives, a 1 over an invalid row does not
    out = torch.ones(R, dtype=torch.uint8, device=DEV)
    out[42] = 0
    again = ops.rows_finite(ts, out=out)
    assert again is out
    w2 = want.copy()
    w2[42] = False
    assert np.array_equal(out.cpu().numpy().astype(bool), w2)


@pytest.mark.gpu
def test_row_scan_at_bases_that_are_not_16_byte_aligned():
    """the matrices as offsets into one buffer: bases 4-byte aligned with every residue mod 16 -- heads of 3, 2, 1 and 0 scalar loads"""
    from dtc_amd import ops
    ms = _matrices()
    want = _want(ms)
    buf = torch.zeros(sum(m.size for m in ms) + 64, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    views, pos, residues = [], 0, set()
    for i, m in enumerate(ms):
        pos += (i % 4) + 1                                   # a gap in front of every matrix
        while (pos % 4) != (i + 1) % 4:                      # matrix i starts at element residue (i + 1) % 4
            pos += 1
        v = buf[pos:pos + m.size].view(R, m.shape[1])
        v.copy_(torch.from_numpy(m))
        residues.add(v.data_ptr() % 16)
        views.append(v)
        pos += m.size
    assert residues == {0, 4, 8, 12}
    assert np.array_equal(ops.rows_finite(views).cpu().numpy().astype(bool), want)
    for m, v in zip(ms, views):
        assert np.array_equal(ops.rows_finite([v]).cpu().numpy().astype(bool), np.isfinite(m).all(1)), (m.shape, v.data_ptr() % 16)


@pytest.mark.gpu
def test_row_scan_past_2_gib():
    """one [400000, 1389] tensor (2.2 GB): a NaN in row 386517, the first row lying wholly past 2^31 bytes, and in the very last element"""
    from dtc_amd import ops
    rows, w = 400000, 1389
    assert 386516 * w * 4 < 2 ** 31 <= 386517 * w * 4
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the test wants 6")
    x = torch.zeros(rows, w, dtype=torch.float32, device=DEV)
    x[386517, 5] = float("nan")
    x[rows - 1, w - 1] = float("nan")
    got = ops.rows_finite([x])
    bad = (got == 0).nonzero().flatten().tolist()
    del x
    assert bad == [386517, rows - 1], bad


# ---------------------------------------------------------------------------------------------------------- contained GAE
T, N = 24, 300                           # two blocks of 256 envs, the second partly filled


def _gae_inputs(dirty):
    rng = np.random.default_rng(23)
    d = dict(rewards=(0.1 * rng.standard_normal((T, N, 1))).astype(np.float32),
             values=(0.5 * rng.standard_normal((T, N, 1))).astype(np.float32),
             dones=(rng.random((T, N, 1)) < 0.05).astype(np.uint8),
             last_values=(0.5 * rng.standard_normal((N, 1))).astype(np.float32))
    d["dones"][22, 9] = 1                # a done between the NaN reward and the end: rows 21..23 of env 9 stay valid either way
    d["dones"][10, 9] = 1                # ... and one the NaN has to cross going backwards (0 * NaN is NaN)
    incoming = np.ones((T, N), dtype=np.uint8)
    if dirty:
        d["rewards"][20, 9, 0] = np.nan
        d["values"][0, 299, 0] = np.inf
        d["last_values"][17, 0] = np.nan
        incoming[7, 5] = 0
    return d, incoming


def _run_default(d):
    from dtc_amd import ops
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    ret, adv = torch.empty(T, N, 1, device=DEV), torch.empty(T, N, 1, device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.gae(t["rewards"], t["values"], t["dones"], t["last_values"], 0.99, 0.95, ret, adv, stats)
    raw = adv.clone()
    return t, ret, adv, raw, stats


def _run_contained(d, incoming):
    from dtc_amd import ops
    t = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    ret, adv = torch.empty(T, N, 1, device=DEV), torch.empty(T, N, 1, device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    rec = torch.from_numpy(incoming.reshape(-1).copy()).to(DEV)
    ops.gae_contained(t["rewards"], t["values"], t["dones"], t["last_values"], 0.99, 0.95, ret, adv, rec, stats)
    raw = adv.clone()
    ops.adv_sqdev_contained(adv, rec, stats)
    ops.adv_normalize_contained(adv, rec, stats)
    return ret, raw, adv, rec, stats


@pytest.mark.gpu
def test_contained_gae_record_statistics_and_normalisation():
    d, incoming = _gae_inputs(dirty=True)
    _t, ret0, _adv0, raw0, _s0 = _run_default(d)
    ret, raw, adv, rec, stats = _run_contained(d, incoming)
    valid = rec.cpu().numpy().reshape(T, N).astype(bool)
    want = np.ones((T, N), dtype=bool)
    want[:21, 9] = False                 # the NaN reward at (20, 9) travels backwards, also across the done at (10, 9)
    want[0, 299] = False                 # inf value: -inf + inf
    want[:, 17] = False                  # NaN bootstrap value
    want[7, 5] = False                   # cleared in the incoming record
    assert np.array_equal(valid, want)
    assert valid[21:, 9].all() and valid[6, 5] and valid[8, 5] and valid[1, 299]
    # valid rows: the bits of ops.gae
    vt = torch.from_numpy(valid).to(DEV).unsqueeze(-1)
    assert torch.equal(ret[vt].view(torch.int32), ret0[vt].view(torch.int32))
    assert torch.equal(raw[vt].view(torch.int32), raw0[vt].view(torch.int32))
    # statistics against float64: the kernels sum exact doubles of the fp32 advantages in another order -- each of the n additions
    # rounds by at most 2^-53 of the running magnitude
    a = raw0.cpu().numpy().reshape(T, N)[valid].astype(np.float64)
    n = a.size
    s = stats.cpu().numpy()
    assert s[1] == n == T * N - 21 - 1 - 24 - 1
    assert abs(s[0] - a.sum()) <= n * 2.0 ** -52 * np.abs(a).sum()
    mean = a.sum() / n
    sq = ((a - mean) ** 2).sum()
    assert abs(s[2] - sq) <= 4 * n * 2.0 ** -52 * sq
    # normalised valid advantages: normalize_kernel restated in float32 on the float64 statistics
    f = np.float32
    mean32, std32 = f(a.sum() / n), f(np.sqrt(sq / (n - 1.0)))
    den = f(std32 + f(1e-8))
    wantn = ((raw0.cpu().numpy().reshape(T, N)[valid].astype(f) - mean32) / den).astype(f)
    gotn = adv.cpu().numpy().reshape(T, N)[valid]
    err = np.abs(gotn.astype(np.float64) - wantn.astype(np.float64)) / np.maximum(1.0, np.abs(wantn.astype(np.float64)))
    print(f"contained normalisation: max error {err.max():.3e} (bound {2.0 ** -21:.3e}), {n} valid rows")
    assert np.isfinite(gotn).all() and err.max() <= 2.0 ** -21


@pytest.mark.gpu
def test_contained_gae_with_every_row_valid_is_the_default_path_bit_for_bit():
    from dtc_amd import ops
    d, incoming = _gae_inputs(dirty=False)
    _t, ret0, adv0, _raw0, s0 = _run_default(d)
    ops.adv_sqdev(adv0, s0, float(T * N))
    ops.adv_normalize(adv0, s0, float(T * N))
    ret, _raw, adv, rec, s = _run_contained(d, incoming)
    assert bool((rec == 1).all())
    assert torch.equal(ret.view(torch.int32), ret0.view(torch.int32))
    assert torch.equal(adv.view(torch.int32), adv0.view(torch.int32))
    s0, s = s0.cpu(), s.cpu()
    assert float(s[1]) == T * N
    assert torch.equal(s[0:1].view(torch.int64), s0[0:1].view(torch.int64))          # sum
    assert torch.equal(s[2:3].view(torch.int64), s0[1:2].view(torch.int64))          # squared deviations


# ---------------------------------------------------------------------------------------------------------- compaction, repair
def _repair_want(perm, valid):
    vl = np.flatnonzero(valid)
    return np.where(valid[perm], perm, vl[perm % len(vl)] if len(vl) else perm), vl


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_bad", [(1536, 30), (300001, 4097)])      # two tiles, the second half full; 293 tiles: runs of 2 in the scan
def test_compaction_and_repair(n, n_bad):
    from dtc_amd import ops
    rng = np.random.default_rng(31)
    valid = np.ones(n, dtype=bool)
    bad = np.concatenate(([0, n - 1], rng.choice(np.arange(1, n - 1), size=n_bad - 2, replace=False)))
    valid[bad] = False
    perm = rng.permutation(n)
    want, vl = _repair_want(perm, valid)
    rec = torch.from_numpy(valid.astype(np.uint8)).to(DEV)
    valid_list, n_valid = ops.compact_valid(rec)
    assert int(n_valid) == len(vl) == n - n_bad
    assert np.array_equal(valid_list.cpu().numpy()[:len(vl)], vl)
    p = torch.from_numpy(perm).to(DEV)
    got = ops.perm_repair(p, rec, valid_list, n_valid)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert valid[got.cpu().numpy()].all() and not valid[perm].all()


@pytest.mark.gpu
def test_repair_with_all_rows_valid_and_with_one():
    from dtc_amd import ops
    n = 1536
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(DEV)
    rec = torch.ones(n, dtype=torch.uint8, device=DEV)
    valid_list, n_valid = ops.compact_valid(rec)
    assert int(n_valid) == n and torch.equal(valid_list, torch.arange(n, device=DEV))
    assert torch.equal(ops.perm_repair(perm, rec, valid_list, n_valid), perm)
    rec.zero_()
    rec[1029] = 1
    valid_list, n_valid = ops.compact_valid(rec)
    assert int(n_valid) == 1 and int(valid_list[0]) == 1029
    assert bool((ops.perm_repair(perm, rec, valid_list, n_valid) == 1029).all())


# ---------------------------------------------------------------------------------------------------------- host checks: no GPU
def test_new_entry_points_reject_bad_arguments_without_gpu():
    """in the manner of tests/test_abi_and_host.py::test_argument_validation_without_gpu: DTC_ERR_ARG and a message, before any
    device work (the non-null pointers below are never dereferenced)"""
    from dtc_amd import _ffi
    lib = _ffi.lib()
    fake = 0x1000

    def scan(ptrs, widths, count, rows, out=fake):
        mats = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        ws = (C.c_int64 * max(1, len(widths)))(*widths)
        return lib.dtc_rows_finite(mats, ws, count, rows, out, None)

    assert scan([fake], [4], 0, 10) == -1 and b"matrices" in lib.dtc_last_error()
    assert scan([fake] * 17, [4] * 17, 17, 10) == -1 and b"matrices" in lib.dtc_last_error()
    assert lib.dtc_rows_finite(None, None, 1, 10, fake, None) == -1 and b"null" in lib.dtc_last_error()
    assert scan([fake], [4], 1, 10, out=None) == -1 and b"null" in lib.dtc_last_error()
    assert scan([fake, None], [4, 4], 2, 10) == -1 and b"null" in lib.dtc_last_error()
    assert scan([fake], [0], 1, 10) == -1 and b"w=0" in lib.dtc_last_error()
    assert scan([fake, fake], [4, -3], 2, 10) == -1 and b"w=-3" in lib.dtc_last_error()
    assert scan([fake], [4], 1, -1) == -1 and b"R=-1" in lib.dtc_last_error()
    assert scan([fake + 2], [4], 1, 10) == -1 and b"aligned" in lib.dtc_last_error()
    assert scan([fake], [4], 1, 0) == 0                                                   # no rows: nothing to do
    assert lib.dtc_gae_contained(None, None, None, None, 0.99, 0.95, None, None, None, None, 24, 64, None) == -1
    assert b"null" in lib.dtc_last_error()
    assert lib.dtc_gae_contained(fake, fake, fake, fake, 0.99, 0.95, fake, fake, None, fake, 24, 64, None) == -1       # the record
    assert lib.dtc_gae_contained(fake, fake, fake, fake, 0.99, 0.95, fake, fake, fake, fake, 0, 64, None) == -1
    assert lib.dtc_adv_sqdev_contained(fake, None, fake, 10, None) == -1
    assert lib.dtc_adv_sqdev_contained(fake, fake, fake, 0, None) == -1
    assert lib.dtc_adv_normalize_contained(fake, fake, None, 10, None) == -1
    assert lib.dtc_compact_valid(None, 10, fake, fake, fake, None) == -1 and b"null" in lib.dtc_last_error()
    assert lib.dtc_compact_valid(fake, 0, fake, fake, fake, None) == -1
    assert lib.dtc_compact_workspace(1536) == 2 * 8 and lib.dtc_compact_workspace(1) == 8
    assert lib.dtc_perm_repair(None, 10, fake, 10, fake, fake, fake, None) == -1 and b"null" in lib.dtc_last_error()
    assert lib.dtc_perm_repair(fake, -1, fake, 10, fake, fake, fake, None) == -1
    assert lib.dtc_perm_repair(fake, 10, fake, -1, fake, fake, fake, None) == -1


def test_wrapper_rejects_bad_matrix_lists():
    from dtc_amd import _ffi, ops
    with pytest.raises(_ffi.DtcError, match="1..16"):
        ops.rows_finite([])
    with pytest.raises(_ffi.DtcError, match="1..16"):
        ops.rows_finite([torch.zeros(4, 2)] * 17)
    with pytest.raises(_ffi.DtcError):
        ops.rows_finite([torch.zeros(4, 2), torch.zeros(5, 2)])
