"""Drop-in ``ConsensusClustering`` (reference: consensus_clustering_parallelised.py, "CC.py").

Same constructor keywords (CC.py:21-36), ``fit(X) -> self`` (CC.py:92-136) and the same
per-K result dict ``cdf_at_K_data[K]`` with keys consensus_labels, hist, cdf, bin_edges,
pac_area, mij, iij, cij and the reference's dtypes (CC.py:378-387): mij/iij in uint8
when n_iterations < 256 else uint16 (CC.py:107), cij float32 with a unit diagonal,
bin_edges float32, hist/cdf float64, pac_area np.float64.

What runs where (``fit``):
  resampling      numpy-RandomState replay on the device (libccmi cc_resample_device /
                  cc_resample_device_wide) or on host threads (cc_resample_indices)
  clustering      default clusterer (KMeans) -> all (h, K, init) problems in batched
                  gfx950 launches (cc_kmeans_batched; in float64 cc_kmeans_f64, which with
                  ``feature_subsampling`` < 1 fits each resample on its own columns,
                  cc_kmeans_f64_cols); AgglomerativeClustering (ward /
                  average / complete, euclidean; average / complete also with
                  manhattan, cosine, correlation) -> one dendrogram per resample on the
                  device, cut at every K (cc_euclidean / cc_pdist, cc_hc_nnchain_batched,
                  cc_hc_cut; ``hierarchical``), with ``feature_subsampling`` < 1 from each
                  resample's own columns (cc_pdist_batched); any other plugin clusterer
                  (e.g. GaussianMixture) keeps the reference's host fit_predict per
                  (K, h) and only its labels go to the GPU (hybrid path); PAM (pam.py, k-medoids
                  under the same four metrics) -> BUILD and SWAP of every (resample, K) on the
                  device over the same distances (cc_pam_build, cc_pam_swap_step, cc_pam_labels);
                  GMM, FullGMM (gmm.py, sklearn's diagonal and full-covariance Gaussian mixtures in
                  float64; gmm_covariance_type_ tells which) -> batched EM of
                  every (resample, K), each init started from the float64 k-means engine's labels
                  (cc_gmm_gather, cc_gmm_start, cc_gmm_em_step, cc_gmm_finish; FullGMM:
                  cc_gmm_full_start, cc_gmm_full_em_step, cc_gmm_full_finish, at most 128 features);
                  NMF (nmf.py, sklearn's NMF(init='random', solver='mu') in float64) -> batched
                  multiplicative updates of every (resample, K), each init from normals drawn on
                  the host and shared by the resamples (cc_gmm_gather, cc_nmf_start, cc_nmf_steps,
                  cc_nmf_finish)
  I, M, histogram int8-MFMA tiles of the upper triangle (cc_cosample / cc_coassoc)
  hist/cdf/PAC    host float64 from 20 exact integer counts (post.py)
  multi-GPU       resamples and triangle tiles sharded over torch.distributed ranks
                  (dist.py); RCCL all-gather of each rank's label columns, SUM of counts

Deliberate differences, all documented in DESIGN.md: the constructor does not delete
files in ``memmap_folder`` (CC.py:83-86); the n x n matrices are materialised only when
``keep_matrices`` (default: n <= 20000) since the reference's O(n^2)-per-K retention is
infeasible at n = 50k; n_jobs / parallelization_method parallelise only the host fits of a
foreign clusterer (``host_fit_predict``: joblib threads or processes as CC.py:185-195, with
labels returned instead of added into a shared Mij, so nothing races; the default KMeans runs on
the GPU whatever n_jobs says).
Additions: ``cdf_area_``, ``delta_k_``, ``pac_area_``, ``best_k_``, ``predict`` and Monti's item and
cluster consensus (``consensus_sums``, ``item_consensus``, ``cluster_consensus``, ``icl``), computed
from the label matrix without the n x n matrices (cc_item_consensus); and the pairwise agreement
of the resamples (``agreement_sums``, ``resample_agreement``, ``partition_agreement``,
``stability``: adjusted Rand / Jaccard on the shared items, cc_agreement_sums).
"""
from __future__ import annotations

import os
import time
import warnings

import numpy as np
import torch

from . import _lib, dist, engine, post
from ._hostfit import fit_predict_chunk, fit_predict_one, subset
from .kmeans import BatchedKMeans
from .pam import METRICS as HC_METRICS  # sklearn's metric spellings -> scipy's names
from .pam import PAM, degenerate_rows as _hc_degenerate, refuse_not_finite
from .pam import validate as _pam_validate
from .gmm import GMM, FullGMM, validate as _gmm_validate
from .nmf import NEGATIVE as _NMF_NEGATIVE, NMF, validate as _nmf_validate

KMAX = 127  # largest K: uint8 labels (0xFF = not sampled) and int8 one-hot channels


def _default_kmeans():
    from sklearn.cluster import KMeans

    return KMeans()


def _is_default_kmeans(est) -> bool:
    """KMeans configured so that the batched gfx950 k-means reproduces it."""
    try:
        from sklearn.cluster import KMeans
    except ImportError:  # pragma: no cover
        return False
    if type(est) is not KMeans:
        return False
    p = est.get_params()
    return (isinstance(p.get("init"), str) and p["init"] == "k-means++"
            and p.get("algorithm", "lloyd") in ("lloyd", "auto", "full")
            and p.get("n_init") is not None)


HC_LINKAGES = ('ward', 'average', 'complete')


PRECISIONS = ('auto', 'f64', 'fast')


def _kmeans_route(precision, wdtype, has_cols):
    """Where the default KMeans runs: (resolved precision, on_device).  precision is the
    constructor keyword (validated here, before it decides anything), wdtype the working dtype of
    X (np.float32 or np.float64), has_cols whether feature subsampling drew a column list.

    'auto' resolves by the input dtype as the reference's clusterer computes in X's dtype
    (CC.py:282): float64 -> 'f64' (cc_kmeans_f64), float32 -> 'fast' (the f16 hi/lo MFMA engines).
    Without columns both run on the device.  With columns only the float64 engine does
    (cc_kmeans_f64_cols gathers each resample's columns in its setup); the float32-class engines
    share one operand image of X across resamples, so 'fast' then keeps the host loop."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'auto', 'f64' or 'fast'")
    if precision == 'auto':
        precision = 'f64' if np.dtype(wdtype) == np.float64 else 'fast'
    return precision, (not has_cols) or precision == 'f64'


def _hc_spec(est):
    """(linkage, metric) of an AgglomerativeClustering that the device trees reproduce (cc_euclidean
    / cc_pdist, cc_hc_nnchain_batched, cc_hc_cut), else None: exactly that type, linkage ward /
    average / complete, no connectivity and no distance threshold.  The metric is scipy's name
    for sklearn's spelling: 'euclidean' ('l2'), 'cityblock' ('manhattan', 'l1'), 'cosine' or
    'correlation'.  Ward goes with euclidean alone (sklearn refuses the rest at fit time, so the
    host path raises its message)."""
    try:
        from sklearn.cluster import AgglomerativeClustering
    except ImportError:  # pragma: no cover
        return None
    if type(est) is not AgglomerativeClustering:
        return None
    p = est.get_params()
    link = p.get("linkage")
    if not isinstance(link, str) or link not in HC_LINKAGES:
        return None
    metric = p.get("metric", "euclidean")
    if metric is None:
        metric = "euclidean"
    if not isinstance(metric, str) or metric not in HC_METRICS:
        return None
    metric = HC_METRICS[metric]
    if link == "ward" and metric != "euclidean":
        return None
    if p.get("connectivity") is not None or p.get("distance_threshold") is not None:
        return None
    return link, metric


def _hc_linkage(est):
    """The linkage of an AgglomerativeClustering that the *euclidean* device trees reproduce
    (cc_euclidean, cc_hc_nnchain_batched, cc_hc_cut), else None: _hc_spec with the euclidean
    metric."""
    spec = _hc_spec(est)
    return spec[0] if spec is not None and spec[1] == "euclidean" else None


def _is_device_hierarchical(est) -> bool:
    """AgglomerativeClustering configured so that the *euclidean* device trees reproduce it."""
    return _hc_linkage(est) is not None


def _hc_route(spec, X, hierarchical, degenerate_test=True):
    """The (linkage, metric) the device trees run, or None for the host loop, from the estimator's
    _hc_spec, the host array X and the ``hierarchical`` keyword; decided from host values alone,
    so every rank decides alike before any launch.  A degenerate row (_hc_degenerate) sends an
    'auto' fit to the host loop, where sklearn raises only if a resample contains the row, and
    is a ValueError under 'device', like an estimator the device does not reproduce.
    degenerate_test=False (feature subsampling, where the device route tests every resample's own
    rows under its own columns) leaves that test out, and X unread."""
    if hierarchical == 'host':
        return None
    if spec is None:
        if hierarchical == 'device':
            raise ValueError("hierarchical='device' needs clusterer=AgglomerativeClustering with linkage "
                             "'ward' (euclidean metric), 'average' or 'complete' (metric 'euclidean', "
                             "'manhattan', 'cosine' or 'correlation'), no connectivity and no "
                             "distance_threshold")
        return None
    # X is read for these two metrics alone (for the others it may be a device tensor)
    why = (_hc_degenerate(np.asarray(X), spec[1]) if degenerate_test and spec[1] in ('cosine', 'correlation')
           else None)
    if why is not None:
        if hierarchical == 'device':
            raise ValueError(why)
        return None
    return spec


def _hc_validate(X, m, Ks):
    """sklearn's own refusals for the device trees, raised from host values before any launch:
    non-finite X (check_array's message; X None = checked elsewhere), fewer than 2 samples per
    resample, and a K above the resample size (_hc_cut's message)."""
    if X is not None:
        X = np.asarray(X)
        refuse_not_finite(X)
        d = X.shape[1] if X.ndim == 2 else 0
    else:
        d = 0
    if m < 2:
        raise ValueError(f"Found array with {m} sample(s) (shape=({m}, {d})) while a minimum of 2 is "
                         "required by AgglomerativeClustering.")
    for K in Ks:
        if K > m:
            raise ValueError("Cannot extract more clusters than samples: "
                             f"{K} clusters were given for a tree with {m} leaves.")


def _int_at_least(v, lo) -> bool:
    """v is an integer (no bool) >= lo."""
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer)) and v >= lo


def _finite_non_negative(v) -> bool:
    """v is a finite real (no bool) >= 0."""
    return (not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
            and bool(np.isfinite(v) and v >= 0))


def _pam_spec(est):
    """scipy's name of the metric of a PAM that the device reproduces (cc_pam_build,
    cc_pam_swap_step, cc_pam_labels), else None: exactly that type (a subclass may override
    anything), a metric of HC_METRICS and an integer max_iter >= 0."""
    if type(est) is not PAM:
        return None
    p = est.get_params()
    metric, max_iter = p.get("metric"), p.get("max_iter")
    if not isinstance(metric, str) or metric not in HC_METRICS:
        return None
    if not _int_at_least(max_iter, 0):
        return None
    return HC_METRICS[metric]


def _pam_route(metric, X):
    """The metric the device PAM runs, or None for the host loop, from _pam_spec and host values
    alone, so every rank decides alike before any launch.  A degenerate row of X
    (_hc_degenerate) keeps the fit in the host loop, where PAM raises only if a resample
    contains the row: the rule of the device trees under hierarchical='auto'.  X None (feature
    subsampling: engine.pam_labels tests every resample's own rows under its own columns)
    leaves that test out."""
    if metric in ('cosine', 'correlation') and X is not None:
        Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        if _hc_degenerate(Xh, metric) is not None:
            return None
    return metric


def _gmm_spec(est):
    """The parameters of a GMM that the device reproduces (cc_gmm_start, cc_gmm_em_step,
    cc_gmm_finish), else None: exactly that type (a subclass may override anything), diagonal
    covariances, integer max_iter >= 1 and n_init >= 1, finite tol >= 0 and reg_covar >= 0."""
    if type(est) is not GMM:
        return None
    p = est.get_params()
    if not isinstance(p.get("covariance_type"), str) or p["covariance_type"] != 'diag':
        return None
    return _em_params(p, ("tol", "reg_covar"))


def _gmm_full_spec(est):
    """_gmm_spec for the full-covariance model (cc_gmm_full_start, cc_gmm_full_em_step,
    cc_gmm_full_finish): exactly the type FullGMM, under the same rules for its parameters."""
    if type(est) is not FullGMM:
        return None
    return _em_params(est.get_params(), ("tol", "reg_covar"))


def _em_params(p, reals):
    """The parameter dict p as the device takes it, else None: integer max_iter >= 1 and
    n_init >= 1, and every parameter named in reals finite and >= 0."""
    if not all(_int_at_least(p.get(name), 1) for name in ("max_iter", "n_init")):
        return None
    if not all(_finite_non_negative(p.get(name)) for name in reals):
        return None
    return dict(n_init=int(p["n_init"]), max_iter=int(p["max_iter"]), **{name: float(p[name]) for name in reals})


def _nmf_spec(est):
    """The parameters of an NMF that the device reproduces (cc_nmf_start, cc_nmf_steps,
    cc_nmf_finish), else None: exactly that type (a subclass may override anything), integer
    max_iter >= 1 and n_init >= 1, finite tol >= 0."""
    if type(est) is not NMF:
        return None
    return _em_params(est.get_params(), ("tol",))


def _to_f64_device(X, dev) -> torch.Tensor:
    """X (a tensor or an array) as a float64 tensor on the device."""
    if isinstance(X, torch.Tensor):
        return X.to(dev, torch.float64)
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)


# what fit() fills for the backend that ran; a refit resets them all first
_RESULT_ATTRS = ('labels_', '_idx_dev', '_idx_host', 'kmeans_inertia_', 'kmeans_n_iter_', 'kmeans_stats_',
                 'hc_stats_', 'hc_metric_', 'pam_stats_', 'pam_metric_', 'pam_inertia_', 'pam_n_iter_',
                 'gmm_stats_', 'gmm_lower_bound_', 'gmm_n_iter_', 'gmm_converged_', 'gmm_covariance_type_',
                 'nmf_stats_', 'nmf_reconstruction_err_', 'nmf_n_iter_', 'nmf_converged_')


class ConsensusClustering:
    """Monti consensus clustering on MI355X.  Drop-in for CC.py:11."""

    def __init__(
        self,
        clusterer=None,
        clusterer_options={'n_init': 3},
        K_range=(2, 3),
        n_iterations=25,
        subsampling=0.8,
        random_state=None,
        consensus_matrix_analysis='PAC',
        PAC_interval=(0.1, 0.9),
        plot_cdf=True,
        agg_clustering_linkage='average',
        n_jobs=1,
        parallelization_method='multithreading',
        memmap_folder='./memmap',
        *,
        keep_matrices='auto',
        device=None,
        workspace_budget=None,
        precision='auto',
        resampling='auto',
        hierarchical='auto',
        feature_subsampling=1.0,
    ):
        self.K_range = K_range
        self.n_iterations = n_iterations
        self.subsampling = subsampling
        self.clusterer = clusterer
        self.clusterer_options = clusterer_options

        self.consensus_matrix_analysis = consensus_matrix_analysis
        self.PAC_interval = PAC_interval
        self.plot_cdf = plot_cdf
        self.agg_clustering_linkage = agg_clustering_linkage

        self.random_state = random_state
        self.n_jobs = n_jobs
        self.parallelization_method = parallelization_method
        self.memmap_folder = memmap_folder  # kept for compatibility; never touched

        self.keep_matrices = keep_matrices
        self.device = device
        self.workspace_budget = workspace_budget
        # k-means arithmetic: 'f64' = float64 like sklearn on float64 input (cc_kmeans_f64),
        # 'fast' = the float32-class f16 hi/lo MFMA engine; 'auto' = f64 for float64 input, fast
        # for float32 (sklearn's own choice of arithmetic follows X's dtype)
        self.precision = precision
        # where the resample indices are drawn: 'device' (cc_resample_device for n <= 65536,
        # cc_resample_device_wide above), 'host' (native threads, then uploaded), 'auto' =
        # device; identical draws
        self.resampling = resampling
        # an AgglomerativeClustering base clusterer (ward / average / complete, euclidean; average /
        # complete also with the manhattan, cosine and correlation metrics): 'auto'
        # = one tree per resample on the device when the estimator is one the device reproduces,
        # 'device' = the same but an error when it is not, 'host' = sklearn's fit_predict per (K, h)
        self.hierarchical = hierarchical
        # the fraction of X's columns each resample sees (ConsensusClusterPlus's pFeature):
        # md = int(feature_subsampling * d) of them, drawn per resample (post.feature_indices);
        # 1.0 = every column, no draw.  The device trees compute each resample's distances from
        # its columns (cc_pdist_batched), the float64 k-means gathers them in its per-resample setup
        # (cc_kmeans_f64_cols); the float32-class k-means engines do not subsample features, so
        # the default KMeans at precision 'fast' then runs in the host loop (_kmeans_route)
        self.feature_subsampling = feature_subsampling
        self.timings_ = {}
        self._rehearsal = None  # (rank, world): bench tooling only, see fit()

        if self.clusterer is None:
            print('KMeans is set as default clusterer')
            self.clusterer = _default_kmeans()

    # ------------------------------------------------------------------ plugin
    def _set_clusterer_K(self):
        """CC.py:201-214: set n_clusters / n_components, then set_params(random_state, **opts)."""
        if hasattr(self.clusterer, 'n_clusters'):
            self.clusterer.n_clusters = self._K
        elif hasattr(self.clusterer, 'n_components'):
            self.clusterer.n_components = self._K
        else:
            raise AttributeError('clusterer has neither n_clusters nor n_components attribute')
        # a deterministic estimator (AgglomerativeClustering, ...) has no random_state to set
        opts = dict(self.clusterer_options)
        get_params = getattr(self.clusterer, 'get_params', None)
        if get_params is None or 'random_state' in get_params():
            opts = dict(random_state=self.random_state, **opts)
        self.clusterer.set_params(**opts)

    def _kmeans_params(self):
        """The KMeans parameters after the reference's set_params (clusterer_options win)."""
        Ks = list(self.K_range)
        if not Ks:
            return None
        self._K = Ks[0]
        self._set_clusterer_K()
        if not _is_default_kmeans(self.clusterer):
            return None
        p = self.clusterer.get_params()
        n_init = p["n_init"]
        if n_init == "auto":
            n_init = 1  # sklearn: 'auto' -> 1 run for init='k-means++'
        return dict(n_init=int(n_init), max_iter=int(p["max_iter"]), tol=float(p["tol"]))

    # ------------------------------------------------------------------ fit
    def fit(self, X):
        """Fit on X [n_samples, n_features] and fill ``cdf_at_K_data`` (CC.py:92-136)."""
        t_start = time.perf_counter()
        if isinstance(X, torch.Tensor):  # already resident in device memory
            wdtype = np.float64 if X.dtype == torch.float64 else np.float32
        else:
            X = np.asarray(X)
            wdtype = X.dtype if X.dtype in (np.float32, np.float64) else np.float64
        self._N, d = X.shape
        self._dtype = np.uint8 if self.n_iterations < 256 else np.uint16
        self.cdf_at_K_data = dict()
        n, H = self._N, int(self.n_iterations)
        m = int(self.subsampling * n)
        Ks = [int(K) for K in self.K_range]
        self._check_k_range(Ks)
        # the reference seeds resample h with random_state + h (CC.py:232): validate the whole
        # H range once, on every rank, before sharding (a rank-local check would let the other
        # ranks go on into the exchanges and hang)
        if self.random_state is None:
            raise TypeError("unsupported operand type(s) for +: 'NoneType' and 'int'")
        if H > 0 and (int(self.random_state) < 0 or int(self.random_state) + H - 1 > 2**32 - 1):
            raise ValueError("Seed must be between 0 and 2**32 - 1")
        # the feature fraction, refused from host values on every rank before any launch or exchange
        md = self._feature_count(d)
        self.feature_indices_ = cols = None
        if md < d:
            self.feature_indices_ = cols = post.feature_indices(self.random_state, d, md, H)
        rank, W = dist.world()
        # a refit replaces the previous results: their device buffers are dropped first, so the
        # new label matrix and indices reuse that memory instead of growing the pool by a set
        for name in _RESULT_ATTRS:
            setattr(self, name, None)
        if self.hierarchical not in ('auto', 'device', 'host'):
            raise ValueError("hierarchical must be 'auto', 'device' or 'host'")
        self.partial_ = False
        if self._rehearsal is not None:
            # one-GPU rehearsal of rank r's share of a W-rank fit (bench tooling only): the
            # exchanges are skipped, so every count below covers rank r's share alone
            if W > 1:
                raise RuntimeError("rehearsal runs without a process group")
            rank, W = self._rehearsal
            self.partial_ = True
            warnings.warn(f"rehearsing rank {rank} of {W}: results are PARTIAL (timing only)")
        dev = engine.require_gpu(self.device)
        keep = self.keep_matrices
        if keep == 'auto':
            keep = n <= 20000

        # resampling (CC.py:216-241): each rank replays only its own resamples [h0, h1); rows
        # outside the shard stay zero and are never read (the co-sampling counts come from the
        # merged label matrix, not from the indices)
        h0, h1 = dist.shard(H, rank, W)
        if self.resampling not in ('auto', 'device', 'host'):
            raise ValueError("resampling must be 'auto', 'device' or 'host'")
        on_dev = self.resampling != 'host'
        self.resampling_ = 'device' if on_dev else 'host'
        idx = None  # host copy, made only when a host consumer needs it (resampling_indices_)
        if on_dev:
            idx_d = (torch.empty if (h0, h1) == (0, H) else torch.zeros)((H, m), dtype=torch.int32, device=dev)
            if h1 > h0:
                engine.resample_indices_device(self.random_state, n, m, h0, h1, dev, out=idx_d[h0:h1])
        else:
            own = engine.resample_indices(self.random_state, n, m, h0, h1) if h1 > h0 else None
            if (h0, h1) == (0, H):
                idx = own
                idx_d = torch.from_numpy(idx).to(dev)
            else:
                idx = np.zeros((H, m), dtype=np.int32)
                idx_d = torch.zeros((H, m), dtype=torch.int32, device=dev)
                if own is not None:
                    idx[h0:h1] = own
                    idx_d[h0:h1] = torch.from_numpy(own).to(dev)
        Hpad = engine.pad_h(H)
        labels = engine.new_label_matrix(max(len(Ks), 1), n, Hpad, dev)
        if on_dev:
            torch.cuda.synchronize(dev)  # stage timing only: the k-means waits for the indices anyway
        t_rs = time.perf_counter()

        km = self._kmeans_params()
        if km is not None and cols is not None and not _kmeans_route(self.precision, wdtype, True)[1]:
            # the float64 engine gathers each resample's columns (cc_kmeans_f64_cols); the
            # float32-class engines share one operand image of X across resamples and do not
            warnings.warn("the k-means engines do not subsample features: with feature_subsampling < 1 the "
                          "KMeans fits run on the host (sklearn, one fit per resample and K) unless they run on "
                          "the float64 engine (float64 input, or precision='f64')", UserWarning)
            km = None
        # the estimator as _kmeans_params left it: clusterer_options applied.  The routes in their
        # order: the first that gives a spec runs, and none of them is the host loop
        routes = (('gpu-kmeans', lambda: km), ('gpu-hc', lambda: self._route_hc(X, cols)),
                  ('gpu-pam', lambda: _pam_route(_pam_spec(self.clusterer), X if cols is None else None)),
                  ('gpu-gmm', lambda: self._route_gmm(md)), ('gpu-nmf', lambda: _nmf_spec(self.clusterer)))
        self.backend_, spec = 'host-clusterer', None
        for name, route in routes if Ks else ():
            spec = route()
            if spec is not None:
                self.backend_ = name
                break
        if self.hierarchical == 'device' and self.backend_ != 'gpu-hc':
            _hc_route(None, None, 'device')  # the trees were not asked (k-means runs, or no K): refused
        precision = self.precision
        if precision == 'auto':
            # the reference's clusterer computes in X's dtype (CC.py:282): float64 input keeps
            # sklearn's float64 arithmetic (cc_kmeans_f64) whatever the size; the float32-class
            # engine is opt-in for it (precision='fast')
            precision = 'f64' if (wdtype == np.float64 and km is not None) else 'fast'
        if precision not in ('f64', 'fast'):
            raise ValueError("precision must be 'auto', 'f64' or 'fast'")
        self.precision_ = precision if km is not None else None
        if km is not None:
            bk = BatchedKMeans(Ks, n_init=km["n_init"], max_iter=km["max_iter"], tol=km["tol"],
                               random_state=self.random_state,
                               workspace_budget=self.workspace_budget)
            self.kmeans_n_iter_ = torch.zeros((len(Ks), H), dtype=torch.int32, device=dev)
            if precision == 'f64':
                # float64 input: the reference's clusterer runs in float64 (CC.py:282)
                X64 = _to_f64_device(X, dev)
                self.kmeans_inertia_ = torch.zeros((len(Ks), H), dtype=torch.float64, device=dev)
                # feature subsampling: every rank holds all H column rows and runs its [h0, h1)
                bk.run_f64(X64.contiguous(), idx_d, n, H, m, h0, h1, labels,
                           inertia=self.kmeans_inertia_, n_iter=self.kmeans_n_iter_,
                           cols_d=None if cols is None else torch.from_numpy(cols).to(dev))
            else:
                if cols is not None:  # _kmeans_route keeps such a fit off these engines
                    raise RuntimeError("the float32-class k-means engines take no column list")
                Xd, xnorm, _, Xhl, sexp = _prepare(X, dev)
                self.kmeans_inertia_ = torch.zeros((len(Ks), H), dtype=torch.float32, device=dev)
                bk.run(Xd, xnorm, X.shape[1], idx_d, n, H, m, h0, h1, labels, weight_dtype=wdtype,
                       inertia=self.kmeans_inertia_, n_iter=self.kmeans_n_iter_, Xhl=Xhl,
                       scale_exp=sexp)
            self.kmeans_stats_ = bk.stats
        elif self.backend_ == 'gpu-hc':
            self.hc_metric_ = spec[1]
            self.hc_stats_ = self._fit_hierarchical(X, wdtype, spec[0], spec[1], idx_d, n, m, h0, h1, Ks, labels, dev,
                                                    cols=cols)
        elif self.backend_ == 'gpu-pam':
            self.pam_metric_ = spec
            self.pam_inertia_ = torch.zeros((len(Ks), H), dtype=torch.float64, device=dev)
            self.pam_n_iter_ = torch.zeros((len(Ks), H), dtype=torch.int32, device=dev)
            self.pam_stats_ = self._fit_pam(X, wdtype, spec, idx_d, n, m, h0, h1, Ks, labels, dev, cols=cols)
        elif self.backend_ == 'gpu-gmm':
            self.gmm_stats_ = self._fit_gmm(X, wdtype, spec, idx_d, n, m, h0, h1, Ks, labels, dev, cols=cols)
        elif self.backend_ == 'gpu-nmf':
            self.nmf_stats_ = self._fit_nmf(X, wdtype, spec, idx_d, n, m, h0, h1, Ks, labels, dev, cols=cols)
        elif Ks:
            if isinstance(X, torch.Tensor):
                X = X.cpu().numpy()
            if idx is None:
                idx = idx_d.cpu().numpy()
            for k, K in enumerate(Ks):
                self._K = K
                self._set_clusterer_K()
                lab = host_fit_predict(self.clusterer, X, idx[h0:h1], self.n_jobs,
                                       self.parallelization_method,
                                       cols=None if cols is None else cols[h0:h1])
                if lab.size and (lab.min() < 0 or lab.max() >= K):
                    raise ValueError(f"clusterer labels must lie in [0, {K})")
                engine.scatter_labels(idx_d[h0:h1].contiguous(), torch.from_numpy(lab).to(dev), n,
                                      labels[k], h_offset=h0)
        dist.merge_labels(labels, H)
        torch.cuda.synchronize(dev)
        t_cl = time.perf_counter()

        # co-sampling, co-association and histogram over this rank's band of tiles
        nt = engine.num_tiles(n)
        t0, t1 = dist.shard(nt, rank, W)
        I_tiles, I_full = engine.cosample(labels[0], n, Hpad, t0, t1, want_full=keep)
        counts = torch.zeros((len(Ks), post.N_BINS), dtype=torch.int64, device=dev)
        M_full = [None] * len(Ks)
        if keep:
            M_full = [torch.zeros((n, n), dtype=torch.int32, device=dev) for _ in Ks]
        engine.coassoc_all(labels, n, Hpad, Ks, t0, t1, I_tiles, counts, M_full if keep else None,
                           streams=int(os.environ.get("CCMI_CO_STREAMS", 3)))
        dist.sum_counts(counts)
        if keep:
            dist.sum_counts(I_full)
            for M in M_full:
                dist.sum_counts(M)
        counts_h = counts.cpu().numpy()
        t_co = time.perf_counter()

        # host post-processing (CC.py:316-387)
        iij = I_full.cpu().numpy().astype(self._dtype) if keep else None
        for k, K in enumerate(Ks):
            hist, cdf, bin_edges, pac_area = post.cdf_from_counts(
                post.pair_counts_to_hist_counts(counts_h[k], n), self.PAC_interval)
            res = dict(consensus_labels=[], hist=hist, cdf=cdf, bin_edges=bin_edges,
                       pac_area=pac_area)
            if keep:
                res['mij'] = M_full[k].cpu().numpy().astype(self._dtype)
                res['iij'] = iij
                res['cij'] = engine.consensus(M_full[k], I_full).cpu().numpy()
            else:
                res['mij'] = res['iij'] = res['cij'] = None
            self.cdf_at_K_data[K] = res
        self.pair_counts_ = {K: counts_h[k] for k, K in enumerate(Ks)}
        self._idx_host, self._idx_dev = idx, idx_d  # rows [h0, h1) of this rank (all at W = 1)
        self.resample_range_ = (h0, h1)
        self.labels_ = labels  # device uint8 [nK, n, Hpad]; 0xFF = not sampled
        self._finish_selection()
        self.timings_ = dict(resample=t_rs - t_start, cluster=t_cl - t_rs,
                             coassoc=t_co - t_cl, post=time.perf_counter() - t_co,
                             total=time.perf_counter() - t_start)
        if self.plot_cdf and rank == 0:
            self._plot_cdf()
        return self

    def _feature_count(self, d):
        """md = int(feature_subsampling * d), the same truncation as the item count; a bool, a
        fraction outside (0, 1] or md < 1 is a ValueError that names the value and d."""
        f = self.feature_subsampling
        ok = not isinstance(f, (bool, np.bool_)) and isinstance(f, (int, float, np.integer, np.floating))
        if ok:
            ok = 0 < f <= 1 and int(f * d) >= 1
        if not ok:
            raise ValueError(f"feature_subsampling must be a fraction in (0, 1] that keeps at least one of the "
                             f"d = {d} features (int(feature_subsampling * d) >= 1), got {f!r}")
        return int(f * d)

    def _fit_hierarchical(self, X, wdtype, link, metric, idx_d, n, m, h0, h1, Ks, labels, dev, cols=None):
        """CC.py:282 for AgglomerativeClustering(linkage=link, metric=metric) on the device: the
        n x n distances once (each rank its own; cc_euclidean, or cc_pdist for 'cityblock',
        'cosine' and 'correlation'), then one tree per resample of [h0, h1), cut at every K, into
        this rank's columns of the label matrix.  Under 'correlation' a device tensor X is copied
        to the host, where numpy centres its rows as scipy does (engine.pdist).

        cols (int32 [H, md], feature subsampling): no n x n matrix; every resample's distances
        come from its own columns (cc_pdist_batched, which centres on the device, so a device
        tensor X stays there for every metric).  A resample that holds a row without distances
        under its columns raises ValueError, as sklearn does in the host loop; the ranks agree on
        the lowest such resample before the label exchange (dist.first_failure), so all raise."""
        nh = max(h1 - h0, 1)
        return self._fit_on_distances(
            X, wdtype, metric, n, m, Ks, dev, cols, _hc_validate,
            lambda budget, md: engine.hc_plan(n, m, nh, len(Ks), budget, md=md),
            lambda Dfull, Xd, cols_d, budget: engine.hc_labels(Dfull, idx_d, h0, h1, Ks, link, labels, budget=budget,
                                                               X=Xd, cols_d=cols_d, metric=metric))

    def _fit_pam(self, X, wdtype, metric, idx_d, n, m, h0, h1, Ks, labels, dev, cols=None):
        """CC.py:282 for PAM(metric=metric, max_iter=...) on the device: the distances as
        _fit_hierarchical takes them (the n x n matrix once, or each resample's own under feature
        subsampling), then BUILD and SWAP of every (resample, K) of [h0, h1) into this rank's
        columns of the label matrix, of pam_inertia_ and of pam_n_iter_ (engine.pam_labels)."""
        nh = max(h1 - h0, 1)
        max_iter = int(self.clusterer.get_params()["max_iter"])
        return self._fit_on_distances(
            X, wdtype, metric, n, m, Ks, dev, cols, _pam_validate,
            lambda budget, md: engine.pam_plan(n, m, nh, len(Ks), max(Ks), budget, md=md),
            lambda Dfull, Xd, cols_d, budget: engine.pam_labels(Dfull, idx_d, h0, h1, Ks, labels, budget=budget,
                                                                max_iter=max_iter, X=Xd, cols_d=cols_d, metric=metric,
                                                                inertia=self.pam_inertia_, n_iter=self.pam_n_iter_))

    def _route_hc(self, X, cols):
        """_hc_route for the estimator.  Under feature subsampling each resample's own rows decide
        (engine.hc_labels finds a row without distances under the resample's columns), so the
        whole-X test is not asked; else it reads host values, for a cosine / correlation estimator
        alone."""
        spec = _hc_spec(self.clusterer)
        if cols is not None:
            return _hc_route(spec, None, self.hierarchical, degenerate_test=False)
        if spec is not None and spec[1] in ('cosine', 'correlation') and isinstance(X, torch.Tensor):
            X = X.detach().cpu().numpy()
        return _hc_route(spec, X, self.hierarchical)

    def _route_gmm(self, md):
        """The parameters of the GMM or FullGMM that the device runs, or None; gmm_covariance_type_
        tells which.  A FullGMM over more than GMM_FULL_MD_MAX features runs in the host loop."""
        spec, self.gmm_covariance_type_ = _gmm_spec(self.clusterer), 'diag'
        if spec is None:
            spec, self.gmm_covariance_type_ = _gmm_full_spec(self.clusterer), 'full'
            if spec is not None and md > engine.GMM_FULL_MD_MAX:
                warnings.warn(f"FullGMM runs on the device for at most {engine.GMM_FULL_MD_MAX} features: with "
                              f"{md} features the fits run on the host (one fit per resample and K)", UserWarning)
                spec = None
        if spec is None:
            self.gmm_covariance_type_ = None
        return spec

    def _fit_gmm(self, X, wdtype, spec, idx_d, n, m, h0, h1, Ks, labels, dev, cols=None):
        """CC.py:282 for GMM(**spec), or FullGMM(**spec) where gmm_covariance_type_ is 'full', on the
        device (_fit_on_rows): EM of every (resample, K) of [h0, h1) into this rank's columns of the
        label matrix, of gmm_lower_bound_, gmm_n_iter_ and gmm_converged_ (engine.gmm_labels).  A
        problem with a variance (a Cholesky pivot under 'full') that is not positive raises
        sklearn's ValueError on every rank."""
        covariance = self.gmm_covariance_type_
        who = "FullGMM" if covariance == 'full' else "GMM"

        def validate(X):
            if isinstance(X, torch.Tensor):
                X = None if bool(torch.isfinite(X).all()) else X.detach().cpu().numpy()
            _gmm_validate(X, m, Ks, who)

        return self._fit_on_rows(
            X, wdtype, dev, cols, idx_d.shape[0], len(Ks), validate,
            lambda budget, md: engine.gmm_plan(n, m, max(h1 - h0, 1), Ks, md, budget, covariance),
            ("GMM", "GaussianMixture"), ('gmm_lower_bound_', 'gmm_n_iter_', 'gmm_converged_'),
            lambda X64, cols_d, value, n_iter, converged: engine.gmm_labels(
                X64, idx_d, h0, h1, Ks, labels, budget=self.workspace_budget, seed=int(self.random_state),
                cols_d=cols_d, lower_bound=value, n_iter=n_iter, converged=converged, covariance=covariance, **spec),
            engine.IllDefinedMixture)

    def _fit_nmf(self, X, wdtype, spec, idx_d, n, m, h0, h1, Ks, labels, dev, cols=None):
        """CC.py:282 for NMF(**spec) on the device (_fit_on_rows; X that is not finite or holds a
        negative entry is refused, a device tensor is tested with torch): the multiplicative
        updates of every (resample, K) of [h0, h1) into this rank's columns of the label matrix,
        of nmf_reconstruction_err_, nmf_n_iter_ and nmf_converged_ (engine.nmf_labels).  No
        problem can fail."""
        def validate(X):
            if not isinstance(X, torch.Tensor):
                return _nmf_validate(X)
            if not bool(torch.isfinite(X).all()):
                refuse_not_finite(X.detach().cpu().numpy())
            if X.numel() and bool((X < 0).any()):
                raise ValueError(_NMF_NEGATIVE)

        return self._fit_on_rows(
            X, wdtype, dev, cols, idx_d.shape[0], len(Ks), validate,
            lambda budget, md: engine.nmf_plan(n, m, max(h1 - h0, 1), Ks, md, budget, spec["n_init"]),
            ("NMF", "NMF"), ('nmf_reconstruction_err_', 'nmf_n_iter_', 'nmf_converged_'),
            lambda X64, cols_d, value, n_iter, converged: engine.nmf_labels(
                X64, idx_d, h0, h1, Ks, labels, budget=self.workspace_budget, seed=int(self.random_state),
                cols_d=cols_d, reconstruction_err=value, n_iter=n_iter, converged=converged, **spec))

    def _fit_on_rows(self, X, wdtype, dev, cols, H, nK, validate, plan, names, outputs, run, failure=None):
        """What the device clusterers over the rows of X share (GMM, FullGMM, NMF): the refusals of
        validate(X) from host values on every rank before any launch, plan(budget, md) when a
        workspace_budget is set (too small: raises before any launch), the warning that a float32
        X is cast (names: ours and sklearn's of the model, which computes in float64 here), the
        [nK, H] outputs (float64 value, int32 n_iter, uint8 converged) under the attribute names
        `outputs`, X as float64 on the device, the column list, and run(X64, cols_d, value, n_iter,
        converged) -> stats.  failure: the exception of run that the ranks agree on
        (dist.first_failure), so that all raise it."""
        validate(X)
        if self.workspace_budget is not None:
            plan(self.workspace_budget, X.shape[1] if cols is None else cols.shape[1])
        if np.dtype(wdtype) != np.float64:
            warnings.warn(f"{names[0]} computes in float64: the float32 X is cast to float64 (sklearn's {names[1]} "
                          "would compute in float32)", UserWarning)
        outs = [torch.zeros((nK, H), dtype=dt, device=dev) for dt in (torch.float64, torch.int32, torch.uint8)]
        for name, t in zip(outputs, outs):
            setattr(self, name, t)
        X64 = _to_f64_device(X, dev).contiguous()
        cols_d = None if cols is None else torch.from_numpy(cols).to(dev)
        if failure is None:
            return run(X64, cols_d, *outs)
        stats = code = None
        try:
            stats = run(X64, cols_d, *outs)
        except failure:
            code = 1
        if dist.first_failure(code, dev) is not None:
            raise failure()
        return stats

    def _fit_on_distances(self, X, wdtype, metric, n, m, Ks, dev, cols, validate, plan, run):
        """What the device clusterers over pdist(X, metric) share (the trees and PAM): the
        refusals of validate(X, m, Ks) from host values, plan(budget, md) when a workspace_budget
        is set (too small: raises before any launch), the distances, and run(Dfull, Xd, cols_d,
        budget) -> stats: with Dfull (float64 [n, n], device) and the rest None, or under feature
        subsampling with Dfull None, the rows Xd on the device and the columns cols_d [H, md]; a
        DegenerateResample of run is then agreed on by the ranks (dist.first_failure)."""
        if isinstance(X, torch.Tensor):
            # a device tensor: the finiteness test runs where X lives (torch, no kernel of ours)
            validate(None if bool(torch.isfinite(X).all()) else X.detach().cpu().numpy(), m, Ks)
            Xd = X.to(dev, torch.float64 if wdtype == np.float64 else torch.float32).contiguous()
        else:
            validate(X, m, Ks)
            Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=wdtype)).to(dev)
        budget = self.workspace_budget
        if budget is not None:
            plan(budget, None if cols is None else cols.shape[1])  # too small: raises before any launch
        if cols is not None:
            cols_d = torch.from_numpy(cols).to(dev)
            stats = code = None
            try:
                stats = run(None, Xd, cols_d, budget)
            except engine.DegenerateResample as e:
                code = e.code
            code = dist.first_failure(code, dev)
            if code is not None:
                raise engine.DegenerateResample(code, metric)
            return stats
        Dfull = engine.euclidean(Xd) if metric == 'euclidean' else engine.pdist(Xd, metric)
        if not bool(torch.isfinite(Dfull).all()):  # finite X can still overflow the squares
            if metric == 'euclidean':
                raise ValueError("the euclidean distances between the rows of X are not all finite "
                                 "(overflow in float64)")
            raise ValueError(f"the {metric} distances between the rows of X are not all finite")
        return run(Dfull, None, None, budget)

    def _check_k_range(self, Ks):
        """Every K of K_range must be an integer in [1, 127] (the uint8 label format and the
        int8 co-association), checked before any clustering runs."""
        for K in Ks:
            if K < 1 or K > KMAX:
                raise ValueError(f"K_range values must lie in [1, {KMAX}], got {K}")

    def _finish_selection(self):
        d = self.cdf_at_K_data
        self.pac_area_ = {K: float(v['pac_area']) for K, v in d.items()}
        self.cdf_area_ = {K: post.cdf_area(v['cdf'], v['bin_edges']) for K, v in d.items()}
        self.delta_k_ = post.delta_k(self.cdf_area_)
        self.best_k_ = post.best_k(self.pac_area_)

    # ------------------------------------------------------------------ extras
    def _device_counts(self, K):
        """int32 M and I (n x n, on the GPU) of one K, recomputed from the fitted label
        matrix (CC.py:264 and :287-290) when the fit did not keep them."""
        if getattr(self, 'labels_', None) is None:
            raise ValueError("fit() first")
        Ks = list(self.cdf_at_K_data)
        k = Ks.index(K)
        n = self._N
        labels = self.labels_
        Hpad = labels.shape[2]
        nt = engine.num_tiles(n)
        I_tiles, I_full = engine.cosample(labels[0], n, Hpad, 0, nt, want_full=True)
        counts = torch.zeros(post.N_BINS, dtype=torch.int64, device=labels.device)
        M = torch.zeros((n, n), dtype=torch.int32, device=labels.device)
        engine.coassoc(labels[k], n, Hpad, K, 0, nt, I_tiles, engine.edges_device(labels.device),
                       counts, M)
        return M, I_full

    def _consensus_device(self, K):
        """float32 C for one K on the device (the kept cij when the fit kept its matrices)."""
        v = self.cdf_at_K_data[K]
        if v.get('cij') is not None:
            return torch.from_numpy(np.ascontiguousarray(v['cij'])).to(self.labels_.device)
        M, I = self._device_counts(K)
        C = engine.consensus(M, I)
        del M, I
        return C

    def consensus_matrix(self, K):
        """float32 C for one K (CC.py:372-373), recomputed on the GPU when not kept."""
        v = self.cdf_at_K_data[K]
        if v.get('cij') is not None:
            return v['cij']
        M, I = self._device_counts(K)
        return engine.consensus(M, I).cpu().numpy()

    def export_memmap(self, folder=None, Ks=None):
        """Write each K's co-association counts as the reference's process-mode file
        (CC.py:147-159): ``<folder>/_temp_{K}``, a raw C-order n x n array of the count dtype
        (uint8 if n_iterations < 256 else uint16), readable with
        ``np.memmap(path, dtype, mode='r', shape=(n, n))``.  Returns {K: path}."""
        import os

        folder = self.memmap_folder if folder is None else folder
        os.makedirs(folder, exist_ok=True)
        out = {}
        for K in (self.cdf_at_K_data if Ks is None else Ks):
            mij = self.cdf_at_K_data[K].get('mij')
            if mij is None:
                mij = self._device_counts(K)[0].cpu().numpy().astype(self._dtype)
            path = os.path.join(folder, f'_temp_{K}')
            mm = np.memmap(path, dtype=self._dtype, shape=(self._N, self._N), mode='w+')
            mm[:] = mij
            mm.flush()
            del mm
            out[K] = path
        return out

    def predict(self, K=None, distance='manhattan'):
        """Consensus labels for K (default ``best_k_``).

        distance='manhattan' (default) is the reference's intended semantics
        (`_get_consensus_labels`, CC.py:292-314): agglomerative clustering with
        ``agg_clustering_linkage`` of the ROWS of C under the manhattan metric
        (``AgglomerativeClustering(n_clusters=K, linkage=..., affinity='manhattan')``, CC.py:306-312;
        sklearn >= 1.4 spells the keyword ``metric``).  Everything runs on the GPU: C from the
        label matrix (cc_coassoc, cc_consensus), the n x n manhattan distances in float64 with
        scipy's summation order (cc_manhattan, bit-identical to
        ``scipy.spatial.distance.pdist(C, 'cityblock')``), and for 'average', 'complete' and
        'weighted' linkage scipy's nn_chain (cc_linkage_nnchain), whose merges the host sorts,
        relabels and cuts as scipy's linkage() and sklearn's ``_hc_cut`` do; for 'single' linkage
        sklearn's own mst_linkage_core (Prim, cc_linkage_mst), sorted and labelled as sklearn's
        linkage_tree does.  n is bounded by HBM (C, then 8 n^2 bytes of distances: 20 GB at
        n = 50 000).

        distance='1-C' is an opt-in variant: the same linkage over 1 - C as a precomputed
        consensus distance.
        """
        K = self.best_k_ if K is None else K
        n = self._N
        link = self.agg_clustering_linkage
        # sklearn's checks (AgglomerativeClustering's parameter validation, check_array's minimum
        # of 2 samples, _hc_cut), raised before any device work
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError("The 'n_clusters' parameter of AgglomerativeClustering must be an int "
                             f"in the range [1, inf) or None. Got {K!r} instead.")
        if n < 2:
            raise ValueError(f"Found array with {n} sample(s) (shape=({n}, {n})) while a minimum of "
                             "2 is required by AgglomerativeClustering.")
        if K > n:
            raise ValueError("Cannot extract more clusters than samples: "
                             f"{K} clusters were given for a tree with {n} leaves.")
        if K not in self.cdf_at_K_data:
            raise KeyError(f"K = {K} is not in K_range of the fit")
        if link == 'ward':
            raise ValueError("ward linkage needs the euclidean metric; the reference's manhattan "
                             "consensus linkage supports 'average', 'complete' and 'single'")
        if distance not in ('manhattan', '1-C'):
            raise ValueError("distance must be 'manhattan' or '1-C'")
        if link in engine.LINKAGE_METHODS or link == 'single':
            C = self._consensus_device(K)
            if distance == 'manhattan':
                D = engine.manhattan(C)
            else:
                D = 1.0 - C.double()
            del C
            Z = engine.linkage_single(D) if link == 'single' else engine.linkage(D, link)
            del D
            return post.hc_cut(K, Z[:, :2].astype(np.int64), n)
        raise ValueError(f"unknown linkage {link!r}: 'average', 'complete', 'weighted' or 'single'")

    # ------------------------------------------------------------------ item / cluster consensus
    def _icl_args(self, K, labels):
        """(K, int64 labels [n], Kc) of the item-consensus methods, validated."""
        if getattr(self, 'labels_', None) is None:
            raise ValueError("fit() first")
        K = self.best_k_ if K is None else K
        if K not in self.cdf_at_K_data:
            raise KeyError(f"K = {K} is not in K_range of the fit")
        if labels is None:
            labels = self.predict(K)
        labels = np.asarray(labels)
        if labels.ndim != 1 or labels.shape[0] != self._N:
            raise ValueError(f"labels must be a 1-d array of length {self._N}, got shape {labels.shape}")
        if labels.dtype.kind not in 'iu':
            raise ValueError("labels must be an integer array")
        if labels.min() < 0 or labels.max() >= KMAX:  # Kc = max + 1 <= 127 (cc_item_consensus)
            raise ValueError(f"labels must lie in [0, {KMAX - 1}]")
        labels = labels.astype(np.int64)
        return K, labels, int(labels.max()) + 1

    def consensus_sums(self, K=None, labels=None):
        """int64 [n, Kc] numpy array S[i, c] = sum over j != i with labels[j] == c of
        C_ij * 2^40, exact, for the consensus matrix C of K (default ``best_k_``) and the
        partition ``labels`` (default ``predict(K)``; any int array of length n with values in
        [0, 126], Kc = max + 1 <= 127, so a partition from elsewhere can be passed where ``predict`` does
        not fit the GPU).  Computed from the fitted label matrix ``labels_`` by the tile kernel
        cc_item_consensus: no n x n matrix is formed, whatever ``keep_matrices`` was.

        Under a torch.distributed process group EVERY rank must call this method (and
        ``item_consensus`` / ``cluster_consensus`` / ``icl``): rank r handles the tiles
        ``dist.shard(num_tiles, r, W)`` and the int64 sums are all-reduced (SUM), so every rank
        returns the one-rank result bit for bit."""
        K, labels, Kc = self._icl_args(K, labels)
        k = list(self.cdf_at_K_data).index(K)
        L = self.labels_
        n, Hpad = self._N, L.shape[2]
        rank, W = dist.world()
        t0, t1 = dist.shard(engine.num_tiles(n), rank, W)
        S = engine.item_consensus_sums(L[k], n, Hpad, K, labels.astype(np.int32), Kc, t0, t1)
        dist.sum_counts(S)
        return S.cpu().numpy()

    def item_consensus(self, K=None, labels=None):
        """float64 [n, Kc]: Monti's item consensus m_i(c), the mean consensus of item i with the
        members of cluster c other than itself (ConsensusClusterPlus calcICL's itemConsensus);
        NaN where c has no other member.  Arguments as ``consensus_sums``."""
        K, labels, Kc = self._icl_args(K, labels)
        return post.item_consensus_from_sums(self.consensus_sums(K, labels), labels, Kc)

    def cluster_consensus(self, K=None, labels=None):
        """float64 [Kc]: Monti's cluster consensus m(c), the mean consensus over the pairs of
        cluster c (calcICL's clusterConsensus); NaN for clusters with fewer than two members.
        Arguments as ``consensus_sums``."""
        K, labels, Kc = self._icl_args(K, labels)
        return post.cluster_consensus_from_sums(self.consensus_sums(K, labels), labels, Kc)

    def icl(self, Ks=None):
        """{K: dict(consensus_labels, item_consensus, cluster_consensus)} for every K of the fit
        (or the given Ks), with ``predict(K)`` as the partition: the whole of calcICL."""
        if getattr(self, 'labels_', None) is None:
            raise ValueError("fit() first")
        out = {}
        for K in (list(self.cdf_at_K_data) if Ks is None else Ks):
            K, labels, Kc = self._icl_args(K, None)
            S = self.consensus_sums(K, labels)
            out[K] = dict(consensus_labels=labels,
                          item_consensus=post.item_consensus_from_sums(S, labels, Kc),
                          cluster_consensus=post.cluster_consensus_from_sums(S, labels, Kc))
        return out

    # ------------------------------------------------------------------ resample agreement
    def agreement_sums(self, K=None, labels=None):
        """The exact contingency sums behind the agreement indices, as an int64 numpy array:
        [H, H, 4] = (s0, s2, r2, c2) for every pair of the H = ``n_iterations`` resamples of K
        (default ``best_k_``) over the items both drew, or, with ``labels`` (an int array of
        length n with ids in [0, 126], as in ``consensus_sums``), [H, 4]: every resample against
        that partition on the items the resample drew.  N[a][b] counts the shared items that the
        first column puts in cluster a and the second in b; s0 = sum N, s2 = sum N^2,
        r2 = sum_a (sum_b N)^2, c2 = sum_b (sum_a N)^2 (``post.agreement_from_sums``).  Computed
        from the fitted label matrix ``labels_`` by cc_agreement_sums; no clustering is rerun.

        Under a torch.distributed process group EVERY rank must call this method (and
        ``resample_agreement`` / ``partition_agreement`` / ``stability``): rank r fills the pairs of
        the tiles ``dist.shard(num_tiles, r, W)`` in a zeroed buffer and the int64 sums are
        all-reduced (SUM), so every rank returns the one-rank result bit for bit."""
        if labels is None:
            if getattr(self, 'labels_', None) is None:
                raise ValueError("fit() first")
            K = self.best_k_ if K is None else K
            if K not in self.cdf_at_K_data:
                raise KeyError(f"K = {K} is not in K_range of the fit")
        else:
            K, labels, Kc = self._icl_args(K, labels)
        k = list(self.cdf_at_K_data).index(K)
        L = self.labels_[k]
        n, H = self._N, int(self.n_iterations)
        rank, W = dist.world()
        if labels is None:
            t0, t1 = dist.shard(engine.agreement_num_tiles(H, K), rank, W)
            S = engine.agreement_sums(L, H, K, n, tile_begin=t0, tile_end=t1)
        else:
            col = torch.from_numpy(labels.astype(np.uint8)).to(L.device)
            t0, t1 = dist.shard(engine.agreement_num_tiles(H, K, 1, Kc), rank, W)
            S = engine.agreement_sums(L, H, K, n, col, 1, Kc, t0, t1)
        dist.sum_counts(S)
        S = S.cpu().numpy()
        return S if labels is None else S[:, 0, :]

    def resample_agreement(self, K=None, index='ari'):
        """float64 [H, H]: the agreement of the clusterings of every two resamples of K (default
        ``best_k_``) on the items both drew: ``index`` 'ari' (sklearn's adjusted_rand_score) or
        'jaccard' (Ben-Hur, Elisseeff & Guyon 2002).  Symmetric, diagonal 1.0; NaN where two
        resamples share fewer than two items."""
        if index not in post.AGREEMENT_INDICES:
            raise ValueError(f"index must be one of {post.AGREEMENT_INDICES}, got {index!r}")
        return post.agreement_from_sums(self.agreement_sums(K), index)

    def partition_agreement(self, K=None, labels=None, index='ari'):
        """float64 [H]: how well each resample's clustering of K matches the partition ``labels``
        (default ``predict(K)``, the consensus partition) on the items that resample drew; a low
        entry marks an outlying resample.  ``labels`` as in ``agreement_sums``."""
        if index not in post.AGREEMENT_INDICES:
            raise ValueError(f"index must be one of {post.AGREEMENT_INDICES}, got {index!r}")
        K, labels, _ = self._icl_args(K, labels)
        return post.agreement_from_sums(self.agreement_sums(K, labels), index)

    def stability(self, Ks=None, index='ari'):
        """{K: mean agreement over the resample pairs h1 < h2} for every K of the fit (or the given
        Ks), NaN entries (pairs sharing fewer than two items) left out; NaN when every entry is.
        The stability criterion of Ben-Hur et al. (2002): a second opinion next to PAC and
        delta-K that costs no extra clustering."""
        if getattr(self, 'labels_', None) is None:
            raise ValueError("fit() first")
        iu = np.triu_indices(int(self.n_iterations), 1)
        out = {}
        for K in (list(self.cdf_at_K_data) if Ks is None else Ks):
            vals = self.resample_agreement(K, index)[iu]
            vals = vals[~np.isnan(vals)]
            out[K] = float(vals.mean()) if vals.size else float('nan')
        return out

    @property
    def resampling_indices_(self):
        """int32 [H, m] host copy of the resample indices (rows [h0, h1) of this rank; copied
        from the device on first access when they were drawn there)."""
        if getattr(self, '_idx_host', None) is None and getattr(self, '_idx_dev', None) is not None:
            self._idx_host = self._idx_dev.cpu().numpy()
        return getattr(self, '_idx_host', None)

    def _plot_cdf(self, ax=None):
        """Consensus CDF per K as a step curve over the bin upper edges, with the PAC interval
        shaded (the ``plot_cdf`` option of CC.py:133-134; presentation only, host matplotlib).
        With no ``ax`` it opens a new figure and shows it, as the reference does; pass ``ax`` to
        draw into an existing figure.  Returns the axes, or None when matplotlib is not
        installed."""
        try:
            import matplotlib.pyplot as plt
        except ImportError:  # pragma: no cover
            return None
        show = ax is None
        if show:
            ax = plt.figure().gca()
        lo, hi = self.PAC_interval
        ax.axvspan(lo, hi, color='0.9', zorder=0)
        for K, res in self.cdf_at_K_data.items():
            upper = np.asarray(res['bin_edges'][1:], dtype=np.float64)
            ax.step(upper, res['cdf'], where='post', label=f'K={K} (PAC {float(res["pac_area"]):.3f})')
        ax.set_xlim(0.0, 1.0)
        ax.set_ylim(0.0, 1.02)
        ax.set_xlabel('consensus value')
        ax.set_ylabel('fraction of pairs <= value')
        ax.legend(fontsize='small')
        if show:
            plt.show()
        return ax


def _clone(clusterer):
    """An independent copy of a plugin clusterer with the same parameters: sklearn's ``clone``
    for estimators (get_params), else a deep copy."""
    if hasattr(clusterer, 'get_params'):
        try:
            from sklearn.base import clone

            return clone(clusterer)
        except Exception:  # not a clonable sklearn estimator
            pass
    import copy

    return copy.deepcopy(clusterer)


def _fit_predict_one(clusterer, Xs):
    return fit_predict_one(clusterer, Xs)


def host_fit_predict(clusterer, X, idx, n_jobs=1, parallelization_method='multithreading', cols=None):
    """int32 labels [len(idx), m] of ``clusterer.fit_predict(X[idx[h]])`` for every resample h
    (CC.py:282), the hybrid path's host stage for a clusterer the GPU k-means does not replace.
    cols: optional int [len(idx), md], the feature subset of each resample (feature subsampling);
    resample h is then fitted on the C-contiguous copy of ``X[idx[h]][:, cols[h]]``.

    n_jobs == 1: one call after the other on the clusterer itself (CC.py:180-183).  Otherwise the
    resamples fan out over joblib workers as CC.py:185-195 does: threads for
    'multithreading', processes for 'multiprocessing' (n_jobs=-1: all cores).  Labels are
    RETURNED, not accumulated into a shared matrix, so the workers cannot race (the reference adds
    into one shared Mij from every worker); under threads each task fits its own copy of the
    clusterer (the reference shares one, whose fit_predict can return another thread's labels).
    A process task carries a contiguous chunk of resamples (about four chunks per worker), and
    its function lives in a module that does not import torch (_hostfit), so a worker starts
    with sklearn alone.

    'multithreading' runs a picklable clusterer on the same process pool: a host fit is GIL-bound
    numpy glue for most foreign clusterers (GaussianMixture's EM measured 1.8x SLOWER on 16
    joblib threads than serially, profiles/r04/rec_r4ai/gmm_time.txt), and the labels do not
    depend on where a fit runs.  A clusterer that cannot be pickled stays on threads, each task
    fitting its own clone.  The labels do not depend on n_jobs or the method as long as the
    clusterer's randomness comes from its random_state, which _set_clusterer_K sets to the int
    seed (CC.py:212) before every K."""
    H = len(idx)
    if H == 0:
        m = idx.shape[1] if getattr(idx, 'ndim', 1) == 2 else 0
        return np.empty((0, m), dtype=np.int32)

    def sub(h):
        return subset(X, idx[h], None if cols is None else cols[h])

    if n_jobs == 1:
        return np.stack([_fit_predict_one(clusterer, sub(h)) for h in range(H)]).astype(np.int32)
    from joblib import Parallel, delayed, effective_n_jobs, parallel_config

    if parallelization_method not in ('multithreading', 'multiprocessing'):
        raise RuntimeError(f'unknown parallelization method: {parallelization_method}')
    if parallelization_method == 'multithreading' and not _picklable(clusterer):
        out = Parallel(n_jobs=n_jobs, prefer='threads')(
            delayed(fit_predict_one)(_clone(clusterer), sub(h)) for h in range(H))
    else:
        chunks = max(1, min(H, 4 * effective_n_jobs(n_jobs)))
        bounds = np.linspace(0, H, chunks + 1).astype(int)
        # one BLAS thread per worker: loky would give each worker cpu_count // n_jobs threads,
        # and cpu_count is the whole machine's on a shared node (16 workers x 16 threads on a
        # 16-CPU share measured 7x slower than the serial loop)
        with parallel_config(backend='loky', inner_max_num_threads=1):
            parts = Parallel(n_jobs=n_jobs)(
                delayed(fit_predict_chunk)(clusterer, [sub(h) for h in range(a, b)])
                for a, b in zip(bounds[:-1], bounds[1:]) if b > a)
        out = [lab for part in parts for lab in part]
    return np.stack(out).astype(np.int32)


def _picklable(obj):
    import pickle

    try:
        pickle.dumps(obj)
        return True
    except Exception:
        return False


def _prepare(X, dev):
    from .kmeans import prepare_rows

    if not isinstance(X, torch.Tensor) and X.dtype.kind != 'f':
        X = np.asarray(X, dtype=np.float64)
    try:
        return prepare_rows(X, dev)
    except _lib.CCMIError as e:
        # cc_prepare_rows refuses non-finite rows before any fit is launched; host arrays and
        # device tensors alike get check_array's message (X is read again on this path only)
        if "non-finite" not in str(e):
            raise
        Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.asarray(X))
        if bool(torch.isnan(Xt).any()):
            raise ValueError("Input X contains NaN.") from e
        dt = str(Xt.dtype).replace("torch.", "")
        raise ValueError(f"Input X contains infinity or a value too large for dtype('{dt}').") from e
