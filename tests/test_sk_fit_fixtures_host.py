"""CPU checks of what the GPU tests of the float32 k-means engines rely on: the n_iter / inertia
fixtures of tests/golden/make_sk_fit_fixtures.py describe the same sklearn fits as the label
fixtures and their emulation of the engines' documented arithmetic stays inside the bound the
engines are held to; the numpy restatement of the row image (tests/row_image_ref.py) is
unambiguous on the inputs tests/test_gpu_row_image.py uses."""
import numpy as np
import pytest

from tests import row_image_ref as R
from tests.sk_parity import load_sk_fixture

FIT_CASES = {"bigk_n1536_d16": 3, "bigk_n1536_d40": 3, "bigk_n1536_d100": 3, "range_n1536_d16": 3,
             "bigk5_n1024_d300": 2, "bigk_n1024_d300": 2, "range_n1024_d300": 2}


def inertia_bound(sigma):
    """|inertia - inertia64| / inertia64 <= 8 sigma + 2^-19: sigma is one float32 rounding per row
    at the magnitude of the cancelling terms, in quadrature (make_sk_fit_fixtures.py); 8 is a tail
    no honest rounding reaches; 2^-19 covers the at most 32-term float32 partial sums of the
    E-step (FLUSH = 32) and the final float32 store."""
    return 8.0 * sigma + 2.0 ** -19


@pytest.mark.parametrize("case", list(FIT_CASES))
def test_fit_fixture_matches_label_fixture_and_bound(case):
    f, lab = load_sk_fixture("fit_" + case), load_sk_fixture(case)
    meta, lmeta = f["meta"], lab["meta"]
    Ks, H = meta["Ks"], meta["H"]
    assert H == FIT_CASES[case] and Ks == lmeta["Ks"] and meta["seed"] == lmeta["seed"] == 7
    assert meta["x_sha256"] == lmeta["x_sha256"] == str(f["x_sha256"])
    assert (meta["frac"], meta["n_init"], meta["threads"]) == (0.8, 3, 1)
    for name, dt in (("n_iter", np.int32), ("exempt", np.bool_), ("inertia64", np.float64), ("sigma", np.float64),
                     ("emu_err", np.float64)):
        assert f[name].shape == (len(Ks), H) and f[name].dtype == dt, name
    # the same fits as the label fixture: classified resamples by their labels, the others by digest
    from tests.conftest import digest

    for k in range(len(Ks)):
        for c, h in enumerate(lmeta["classify"]):
            assert f["digest"][k, h] == digest(lab["ref32"][k, c]), (case, Ks[k], h)
        for c, h in enumerate(lmeta["ref"]):
            assert f["digest"][k, h] == lab["ref_digest"][k, c], (case, Ks[k], h)
    assert sorted(lmeta["classify"] + lmeta["ref"]) == list(range(H))
    assert np.all(f["n_iter"] >= 1) and np.all(f["n_iter"] < 300)
    assert f["exempt"].mean() <= 0.05
    assert np.all(f["inertia64"] > 0) and np.all(f["sigma"] > 0)
    # the documented arithmetic itself stays inside the bound
    rel = np.abs(f["emu_err"]) / f["inertia64"]
    assert np.all(rel <= inertia_bound(f["sigma"])), (case, float((rel / inertia_bound(f["sigma"])).max()))


def test_xnorm_emulation_flags_double_rounding():
    """The one case where rounding q + v v to float64 and then to float32 differs from fmaf's single
    rounding is flagged: an inexact float64 sum that lands on a float32 midpoint.  4097^2 =
    2^24 + 8193 is a 25-bit odd integer, half way between two float32 values; 2^-40 more lies
    above the midpoint (fmaf gives 2^24 + 8194), but float64 drops it and the tie goes to even."""
    mids = np.array([1.0 + 2.0 ** -24, 2.0 + 3.0 * 2.0 ** -24, 2.0 ** 20 + 2.0 ** -4, 16785409.0, 1.0,
                     1.0 + 2.0 ** -23, 1.0 + 2.0 ** -24 + 2.0 ** -52])
    assert R._f32_midpoint(mids).tolist() == [True, False, True, True, False, False, False]
    rows = np.array([[2.0 ** -20, 4097.0],     # inexact and on the midpoint: flagged
                     [0.0, 4097.0],            # the midpoint itself, exact: one rounding, ties to even
                     [1.0, 2.0 ** -12],        # 1 + 2^-24, likewise
                     [3.0, 0.5],               # exact
                     [1.0, 2.0 ** -30]],       # inexact in float64, far from a midpoint
                    dtype=np.float32)
    q, amb = R.xnorm_fma(rows)
    assert amb.tolist() == [True, False, False, False, False]
    assert q.tolist() == [16785408.0, 16785408.0, 1.0, 9.25, 1.0]


def test_row_image_inputs_leave_no_row_ambiguous():
    """The inputs of tests/test_gpu_row_image.py: the one-rounding xnorm emulation is unambiguous
    on every row (the GPU test allows 1 %), hi stays within 2^14, the exponent inside its clamp,
    and each data family has the property it is there for."""
    for n, d in R.SHAPES:
        for kind in R.KINDS:
            ref = R.row_image(R.make_rows(kind, n, d))
            what = (kind, n, d)
            assert not ref["ambiguous"].any(), what
            assert -62 < ref["e"] < 62, what
            assert np.abs(ref["hi"].astype(np.float64)).max() <= 2.0 ** 14, what
            assert np.all(np.isfinite(ref["xnorm"])), what
            if n == 1:
                assert not ref["Xd"].any() and ref["e"] == 0, what
                continue
            if kind == "offset":   # centring cancels: |Xd| is four decimal orders below |X|
                assert ref["amax"] < 8 and abs(float(ref["mean"][0]) - 1e4) < 1, what
            if kind == "constant":
                assert not ref["Xd"][:, 0].any(), what
            if kind in ("pow2", "pow2_ulp"):
                assert ref["mean"][0] == 0, what
                assert ref["amax"] == (8.0 if kind == "pow2" else float(np.nextafter(np.float32(8), np.float32(16)))), what
                assert ref["e"] == (11 if kind == "pow2" else 10), what
                top = np.abs(ref["hi"].astype(np.float64)).max()
                assert top == (2.0 ** 14 if kind == "pow2" else 2.0 ** 13), what


def test_scale_exponent_rule():
    for amax, e in ((0.0, 0), (1.0, 14), (2.0 ** 14, 0), (np.nextafter(np.float32(2.0 ** 14), np.float32(1e9)), -1),
                    (3.0, 12), (2.0 ** -100, 62), (2.0 ** 100, -62), (np.float32(0.75), 14)):
        assert R.scale_exponent(amax) == e, amax
