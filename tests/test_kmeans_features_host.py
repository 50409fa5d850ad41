"""Feature subsampling on the float64 k-means, the parts that need no GPU: which fits go to the
device (api._kmeans_route), the new entry point in the header and the library, the committed
sklearn fixtures (tests/golden/make_sk_feature_fixtures.py) and the planner at the subset's width.
tests/test_gpu_kmeans_features.py runs the kernels."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from consensus_clustering_amd import _lib, api, kmeans, post
from tests.sk_parity import load_sk_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case: n, d, md, Ks, H (the issue's table; md = int(fraction * d))
FEATURE_CASES = {
    "n600_d12": (600, 12, 9, [2, 3, 4, 6, 9], 4),
    "n29_d29": (29, 29, 23, [2, 3, 4, 5, 6, 7, 8, 9, 10], 6),
    "n300_d150": (300, 150, 120, [2, 3, 5], 3),
    "n200_d4": (200, 4, 3, [2, 3, 5], 4),
}


@pytest.mark.parametrize("precision,wdtype,has_cols",
                         list(itertools.product(api.PRECISIONS, (np.float32, np.float64), (False, True))))
def test_route_of_every_combination(precision, wdtype, has_cols):
    resolved, on_device = api._kmeans_route(precision, wdtype, has_cols)
    want = precision if precision != "auto" else ("f64" if wdtype == np.float64 else "fast")
    assert resolved == want
    # without columns nothing changes; with them only the float64 engine fits on the device
    assert on_device == ((not has_cols) or want == "f64")
    assert api._kmeans_route(precision, np.dtype(wdtype), has_cols) == (resolved, on_device)


@pytest.mark.parametrize("bad", ["F64", "double", None, 64, ""])
@pytest.mark.parametrize("has_cols", [False, True])
def test_route_validates_the_keyword_first(bad, has_cols):
    for wdtype in (np.float32, np.float64):
        with pytest.raises(ValueError, match="precision must be 'auto', 'f64' or 'fast'"):
            api._kmeans_route(bad, wdtype, has_cols)


def test_header_declares_and_library_exports_the_entry():
    src = open(os.path.join(ROOT, "include", "ccmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    proto = re.search(r"\bint\s+cc_kmeans_f64_cols\s*\(([^)]*)\)\s*;", code)
    assert proto, "include/ccmi.h does not declare cc_kmeans_f64_cols"
    args = [a.strip() for a in proto.group(1).split(",")]
    plain = re.search(r"\bint\s+cc_kmeans_f64\s*\(([^)]*)\)\s*;", code)
    plain_args = [a.strip() for a in plain.group(1).split(",")]
    # X, n, d, then the column list and its width, then cc_kmeans_f64's own list from idx_hm on
    assert args[:3] == plain_args[:3]
    assert args[3:5] == ["const int32_t* cols_hmd", "int md"]
    assert args[5:] == plain_args[3:]
    assert "cc_kmeans_f64_cols" in re.search(r"/\*.*?\*/", src, flags=re.S).group(0)  # the header's list of entries
    lib = _lib.load()
    assert hasattr(lib, "cc_kmeans_f64_cols")
    res, argtypes = _lib.SIGNATURES["cc_kmeans_f64_cols"]
    assert res is ctypes.c_int and len(argtypes) == len(args) == len(_lib.SIGNATURES["cc_kmeans_f64"][1]) + 2
    assert lib.cc_kmeans_f64_cols.argtypes == argtypes


@pytest.mark.parametrize("case", list(FEATURE_CASES))
def test_fixture_loads_and_its_columns_are_the_drawn_ones(case):
    n, d, md, Ks, H = FEATURE_CASES[case]
    f = load_sk_fixture("f64_feat_" + case)
    meta = f["meta"]
    assert (meta["n"], meta["d"], meta["md"], meta["Ks"], meta["H"], meta["seed"]) == (n, d, md, Ks, H, 3)
    assert md == int(meta["fraction"] * d) and meta["relocated_rows"] == 0
    m = int(0.8 * n)
    assert f["labels"].dtype == np.int8 and f["labels"].shape == (len(Ks), H, m)
    assert f["cols"].dtype == np.int32
    np.testing.assert_array_equal(f["cols"], post.feature_indices(3, d, md, H))
    assert (np.diff(f["cols"], axis=1) > 0).all()
    assert f["n_iter"].shape == f["inertia"].shape == f["digest64"].shape == (len(Ks), H)
    assert (f["n_iter"] >= 1).all() and (f["inertia"] > 0).all()
    from tests.conftest import digest

    for k, K in enumerate(Ks):
        for h in range(H):
            assert digest(f["labels"][k, h]) == f["digest64"][k, h]
            assert sorted(set(f["labels"][k, h].tolist())) == list(range(K))


@pytest.mark.parametrize("case", list(FEATURE_CASES))
@pytest.mark.parametrize("cus,nh_of", [(256, lambda H: H), (8, lambda H: 1)])
def test_planner_at_the_subset_width(case, cus, nh_of):
    """A fit on md columns is planned like a plain fit of d = md: one float64 call whose workspace
    is cc_kmeans_f64_workspace_bytes at width md (the slots hold md columns), never X's width."""
    n, d, md, Ks, H = FEATURE_CASES[case]
    m, nh = int(0.8 * n), nh_of(H)
    args = (m, nh, Ks, 3, 1, cus, kmeans.UNLIMITED, kmeans.UNLIMITED)
    sub, full = kmeans.launch_plan(md, *args), kmeans.launch_plan(d, *args)
    assert [c["engine"] for c in sub] == ["cc_kmeans_f64"] and (sub[0]["k0"], sub[0]["nk"]) == (0, len(Ks))
    assert sub[0]["par"] == full[0]["par"]  # the grid follows the units, not the width
    Ks_np = np.asarray(Ks, dtype=np.int32)
    lib = _lib.load()

    def need(width, grid):
        return int(lib.cc_kmeans_f64_workspace_bytes(m, width, Ks_np.ctypes.data, len(Ks), grid, nh))

    assert sub[0]["ws_bytes"] == need(md, sub[0]["par"])
    assert full[0]["ws_bytes"] == need(d, full[0]["par"])
    assert sub[0]["ws_bytes"] < full[0]["ws_bytes"]
