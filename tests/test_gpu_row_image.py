"""The row image every float32 fit consumes (cc_prepare_rows: colsum_kernel, colmean_kernel,
centre_kernel; cc_split_f16: split_kernel) against a numpy restatement in the kernels' stated
order (tests/row_image_ref.py): column means, centred padded rows, squared norms, the scale
exponent and the f16 hi/lo operand image, read back from the device and compared bit for bit.

Shapes: n in {1, 255, 256, 257, 513} (one row, either side of the 256-row column-sum and centring
blocks, a third block) and d in {1, 31, 32, 33, 100, 128, 129, 300} (either side of each padded
width, the wide engine's multiple of 32, and the second trip of the 256-thread column loop);
every n with one narrow and one wide d, every d with n = 257.  Data: row_image_ref.make_rows.

Non-finite input must be refused by cc_prepare_rows itself: for a device tensor and for the C ABI
it is the only guard in front of the fit."""
import ctypes

import numpy as np
import pytest
import torch

from consensus_clustering_amd import ConsensusClustering, _lib, engine, kmeans
from tests import row_image_ref as R

pytestmark = pytest.mark.gpu

CC_ERR_ARG = -1


def device_image(X, dpad=None):
    """cc_prepare_rows on X with every output and the scratch pre-filled with non-zero patterns.
    Returns (rc, dict of host arrays)."""
    dev = engine.require_gpu()
    lib = _lib.load()
    n, d = X.shape
    dpad = lib.cc_kmeans_dpad(d) if dpad is None else dpad
    Xt = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(dev)
    Xd = torch.full((n, dpad), 7.5, dtype=torch.float32, device=dev)
    xnorm = torch.full((n,), -3.0, dtype=torch.float32, device=dev)
    Xhl = torch.full((n, 2, dpad), 0x3C5A, dtype=torch.int16, device=dev)
    scratch = torch.full((int(lib.cc_prepare_rows_scratch_bytes(n, d)),), 0xA5, dtype=torch.uint8, device=dev)
    e = ctypes.c_int(12345)
    rc = lib.cc_prepare_rows(Xt.data_ptr(), n, d, dpad, Xd.data_ptr(), xnorm.data_ptr(), Xhl.data_ptr(),
                             ctypes.byref(e), scratch.data_ptr(), scratch.numel(), engine.stream_ptr(dev))
    torch.cuda.synchronize()
    nb = (n + R.RB - 1) // R.RB
    mean_off = (nb * d * 8 + 255) // 256 * 256  # fit.hip: the means follow the column partials
    mean = scratch[mean_off:mean_off + 4 * d].cpu().numpy().view(np.float32)
    hl = Xhl.cpu().numpy().view(np.float16)
    return rc, dict(mean=mean, Xd=Xd.cpu().numpy(), xnorm=xnorm.cpu().numpy(), hi=hl[:, 0], lo=hl[:, 1],
                    e=int(e.value), dpad=dpad)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def check_image(X, got, what, left_out):
    n, d = X.shape
    ref = R.row_image(X, got["dpad"])
    dpad = ref["dpad"]
    np.testing.assert_array_equal(bits(got["mean"]), bits(ref["mean"]), err_msg=f"{what}: mean")
    np.testing.assert_array_equal(bits(got["Xd"]), bits(ref["Xd"]), err_msg=f"{what}: Xd")
    # padding: exactly +0 in Xd and in both halves of the image (the buffers were pre-filled)
    assert not bits(got["Xd"])[:, d:].any() and not bits(got["hi"])[:, d:].any() and not bits(got["lo"])[:, d:].any(), what
    # xnorm: bit for bit wherever the one-rounding emulation is unambiguous; always within
    # dpad 2^-24 relative of the float64 sum of squares (dpad sequential roundings of a growing sum)
    ok = ~ref["ambiguous"]
    left_out[0] += int(ref["ambiguous"].sum())
    left_out[1] += n
    np.testing.assert_array_equal(bits(got["xnorm"])[ok], bits(ref["xnorm"])[ok], err_msg=f"{what}: xnorm")
    ss = (ref["Xd"].astype(np.float64) ** 2).sum(axis=1)
    assert np.all(np.abs(got["xnorm"].astype(np.float64) - ss) <= dpad * 2.0 ** -24 * ss), what
    # scale exponent: the library's own rule at the reference's max |Xd|, the same in integer
    # arithmetic, and what it is for: every hi finite with |hi| <= 2^14
    e = ctypes.c_int(0)
    _lib.call("cc_scale_exponent", ctypes.c_float(ref["amax"]), ctypes.byref(e))
    assert got["e"] == e.value == ref["e"], (what, got["e"], e.value, ref["e"])
    assert -62 <= got["e"] <= 62
    hi64 = got["hi"].astype(np.float64)
    assert np.all(np.isfinite(hi64)) and np.abs(hi64).max(initial=0.0) <= 2.0 ** 14, what
    if ref["amax"] > 0 and -62 < got["e"] < 62:  # not clamped: the image uses the top binade
        assert np.abs(hi64).max() > 2.0 ** 12, (what, np.abs(hi64).max())
    # the image, including f16-subnormal and zero lo halves and the sign of zero
    np.testing.assert_array_equal(bits(got["hi"]), bits(ref["hi"]), err_msg=f"{what}: hi")
    np.testing.assert_array_equal(bits(got["lo"]), bits(ref["lo"]), err_msg=f"{what}: lo")
    # reconstruction: hi + lo carries Xd 2^e to 2^-22 of the largest operand
    xs = ref["Xd"].astype(np.float64) * 2.0 ** got["e"]
    assert np.abs(hi64 + got["lo"].astype(np.float64) - xs).max(initial=0.0) <= 2.0 ** -22 * 2.0 ** 14, what
    return ref


@pytest.mark.parametrize("n,d", R.SHAPES)
def test_row_image_matches_numpy(n, d):
    left_out = [0, 0]
    for kind in R.KINDS:
        X = R.make_rows(kind, n, d)
        rc, got = device_image(X)
        assert rc == 0, (kind, _lib.load().cc_last_error())
        assert got["dpad"] == R.dpad_for(d)
        ref = check_image(X, got, f"{kind} n={n} d={d}", left_out)
        if kind == "constant" and n > 1:
            assert not bits(got["Xd"])[:, 0].any()                       # exact +0
            if d > 2:                                                    # a -0.0 column stays -0
                assert np.all(bits(got["Xd"])[:, d - 1] == 0x80000000) and np.all(bits(got["hi"])[:, d - 1] == 0x8000)
        if kind == "tiny_column" and n > 1 and d > 1:
            lo = ref["lo"][:, d // 2]
            assert np.all(np.abs(lo.astype(np.float64)) < 2.0 ** -14) and (bits(lo) & 0x7FFF).any()  # subnormal lo
        if kind in ("pow2", "pow2_ulp") and n > 1:
            assert ref["mean"][0] == 0 and ref["amax"] == float(X[:, 0].max())
            assert ref["e"] == (11 if kind == "pow2" else 10)
        if kind in ("huge", "small") and n > 1:
            assert abs(ref["e"] - (14 + (-40 if kind == "huge" else 40))) <= 4
    assert left_out[0] <= 0.01 * left_out[1], left_out
    print(f"row image n={n} d={d}: {left_out[0]} of {left_out[1]} rows left out of the xnorm bit comparison")


@pytest.mark.parametrize("n,d,dpad", [(257, 31, 64), (257, 100, 160), (1, 33, 33), (513, 1, 32)])
def test_row_image_at_a_caller_chosen_dpad(n, d, dpad):
    """cc_prepare_rows takes any dpad >= d (cc_kmeans_fit passes the planner's): the padding and
    the row stride follow it."""
    left_out = [0, 0]
    for kind in ("normal", "offset"):
        X = R.make_rows(kind, n, d, seed=1)
        rc, got = device_image(X, dpad)
        assert rc == 0
        check_image(X, got, f"{kind} n={n} d={d} dpad={dpad}", left_out)
    assert left_out[0] == 0


@pytest.mark.parametrize("e", [-62, -30, 0, 50, 62])
def test_split_f16_at_given_exponents(e):
    """cc_split_f16 alone, at exponents a fit's own data would not reach together with these
    magnitudes: values whose scaled image spans f16's normal, subnormal and zero ranges."""
    dev = engine.require_gpu()
    rng = np.random.default_rng(e + 100)
    n, dpad = 257, 96
    mag = 2.0 ** rng.integers(-30, 14, size=(n, dpad))
    Xd = (rng.normal(size=(n, dpad)) * mag * 2.0 ** -e / 4).astype(np.float32)
    Xd[0, :4] = [0.0, -0.0, 2.0 ** (14 - e), -2.0 ** (14 - e)]
    Xhl = torch.full((n, 2, dpad), 0x3C5A, dtype=torch.int16, device=dev)
    Xt = torch.from_numpy(Xd).to(dev)
    _lib.call("cc_split_f16", Xt.data_ptr(), n, dpad, e, Xhl.data_ptr(), engine.stream_ptr(dev))
    torch.cuda.synchronize()
    hl = Xhl.cpu().numpy().view(np.float16)
    hi, lo = R.split_f16(Xd, e)
    assert np.all(np.isfinite(hi.astype(np.float64)))
    np.testing.assert_array_equal(bits(hl[:, 0]), bits(hi))
    np.testing.assert_array_equal(bits(hl[:, 1]), bits(lo))


BAD = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("bad", list(BAD))
def test_non_finite_rows_are_refused(n, bad):
    """One NaN, +inf or -inf in X: CC_ERR_ARG with "non-finite" in cc_last_error(), wherever it
    sits (first row, last row, the column next to the padding).  Only cc_prepare_rows runs."""
    d = 33
    places = sorted({(0, 0), (n - 1, 5), (n // 2, d - 1), (n - 1, d - 1)})
    for r, c in places:
        X = R.make_rows("normal", n, d, seed=2)
        X[r, c] = BAD[bad]
        rc, _ = device_image(X)
        msg = _lib.load().cc_last_error().decode()
        assert rc == CC_ERR_ARG and "non-finite" in msg, (bad, n, (r, c), rc, msg)
    rc, _ = device_image(R.make_rows("normal", n, d, seed=2))  # and the same rows without it pass
    assert rc == 0


def test_fit_refuses_nan_in_a_device_tensor():
    """ConsensusClustering.fit on a device tensor with a NaN: refused by cc_prepare_rows before
    any fit is launched, with the ValueError a host array gets (check_array's message)."""
    dev = engine.require_gpu()
    X = R.make_rows("normal", 257, 33, seed=3)
    X[200, 7] = np.nan
    with pytest.raises(_lib.CCMIError, match="non-finite"):  # the guard itself, first
        kmeans.prepare_rows(torch.from_numpy(X).to(dev), dev)
    for rows in (X, torch.from_numpy(X).to(dev)):
        cc = ConsensusClustering(K_range=[2, 3], n_iterations=4, subsampling=0.8, random_state=1, plot_cdf=False)
        with pytest.raises(ValueError, match=r"Input X contains NaN\."):
            cc.fit(rows)
    Xi = R.make_rows("normal", 257, 33, seed=3)
    Xi[0, 0] = np.inf
    cc = ConsensusClustering(K_range=[2, 3], n_iterations=4, subsampling=0.8, random_state=1, plot_cdf=False)
    with pytest.raises(ValueError, match=r"Input X contains infinity"):
        cc.fit(torch.from_numpy(Xi).to(dev))
