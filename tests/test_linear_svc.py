"""``classification.LinearSVC`` / ``LinearSVCModel``: fits against sklearn's dual solver, the API, and
two gloo ranks against one.

Objective: f(w, b) = 1/m sum_r l(y'_r z_r) + regParam/2 ||q w||^2, q = sigma (unbiased column std)
with ``standardization`` and 1 without. The datasets are those of the issue's CPU probe: seed-0
standard-normal X (m x n), labels sign(X w_t + noise eps), (m, n, regParam, noise) in ``DATASETS``.
Oracle: sklearn ``LinearSVC(dual=True, C=1/(m regParam), fit_intercept=False, tol=1e-10)`` on X / q,
which minimises the same objective when there is no intercept.

Squared hinge: f is regParam-strongly convex in u = q w, so
||u - u*|| <= (||grad f(u)|| + ||grad f(u*)||) / regParam, both gradients recomputed in fp64 here.

Hinge (non-smooth; the L-BFGS usually runs to maxIter): the relative gap g = (f - f*) / f*. The CPU
path is held to g <= 1e-4; the device may exceed the CPU path's gap on the same data by a factor of 3
(the two run the same state machine and differ by the data term's rounding, which sends a line
search on a non-smooth objective down another branch). Measured gaps, CPU path / MI355X
(``fused_svc_f32``): 2000 x 20: 1.04e-5 / 1.66e-5; 3000 x 64: 4.17e-6 / 4.23e-6; 500 x 8: 2.65e-5 / 2.65e-5.

Two ranks against one (gloo ranks on the CPU path): within the strong-convexity bound, and, under
SRML_DETERMINISTIC=1, bit-equal: the host path then sums the column moments and the data term on a
fixed-point grid (``ops.exact_sum``), on which two partial sums and an all-reduce add up to the
one-rank sum exactly. (With ordinary fp64 sums the two models differed by 2.78e-17, one unit in the
last place of a coefficient.)
"""
import numpy as np
import pytest

from spark_rapids_ml_nai_amd import DataFrame
from spark_rapids_ml_nai_amd.classification import LinearSVC, LinearSVCModel
from spark_rapids_ml_nai_amd.evaluation import MulticlassClassificationEvaluator
from test_svc_kernels import U32, U64, bounds, reference

DATASETS = [(2000, 20, 0.01, 0.5), (3000, 64, 0.1, 2.0), (500, 8, 0.001, 0.2)]
IDS = ["2000x20", "3000x64", "500x8"]


def data(m, n, noise, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, n))
    wt = rng.standard_normal(n)
    y = (X @ wt + noise * rng.standard_normal(m) > 0).astype(np.float64)
    return X.astype(np.float32), y


def objective(Xd, y, u, b, reg, squared):
    """(f, grad_u, grad_b) in fp64 at coefficients u of the columns Xd (already divided by q)."""
    s = 2 * y - 1
    h = 1 - s * (Xd @ u + b)
    act = h > 0
    r = np.where(act, -2 * s * h if squared else -s, 0.0)
    l = np.where(act, h * h if squared else h, 0.0)
    m = len(y)
    return l.mean() + 0.5 * reg * u @ u, r @ Xd / m + reg * u, r.sum() / m


_sk_cache = {}


def sk_optimum(i, squared, standardization):
    """sklearn's solution u* (coefficients of X / q), computed once per (dataset, loss, scaling)."""
    key = (i, squared, standardization)
    if key not in _sk_cache:
        from sklearn.svm import LinearSVC as SkSVC

        m, n, reg, noise = DATASETS[i]
        X, y = data(m, n, noise)
        Xd, q = scaled(X, standardization)
        sk = SkSVC(loss="squared_hinge" if squared else "hinge", dual=True, C=1.0 / (m * reg), fit_intercept=False,
                   tol=1e-10, max_iter=5_000_000).fit(Xd, y)
        _sk_cache[key] = sk.coef_[0].copy()
    return _sk_cache[key]


def scaled(X, standardization):
    Xd = X.astype(np.float64)
    q = Xd.std(0, ddof=1) if standardization else np.ones(X.shape[1])
    return Xd / q, q


def data_term_tol(Xd, y, u, b, squared, path):
    """The kernel bound of tests/test_svc_kernels.py on [grad | grad_b | loss] at (u, b), per row count."""
    cls = {"torch-cpu": (U64, U64), "fused_svc_f32": (U64, U32)}[path]
    ref = reference(Xd, y, u, b, squared)
    try:
        return bounds(ref, *cls) / len(y)
    except AssertionError:  # a hinge row within dz of the kink: no bound to offer
        return None


def fit(i, loss, standardization, fit_intercept=False, **kw):
    m, n, reg, noise = DATASETS[i]
    X, y = data(m, n, noise)
    model = LinearSVC(regParam=reg, fitIntercept=fit_intercept, standardization=standardization, loss=loss, maxIter=100,
                      tol=1e-6, **kw).fit(DataFrame.from_numpy(X, y))
    return X, y, reg, model


def check_squared_hinge(i, standardization, path):
    X, y, reg, model = fit(i, "squared_hinge", standardization)
    assert model._solver_info["path"] == path
    Xd, q = scaled(X, standardization)
    u, us = np.asarray(model.coef_) * q, sk_optimum(i, True, standardization)
    f, g, _ = objective(Xd, y, u, 0.0, reg, True)
    fs, gs, _ = objective(Xd, y, us, 0.0, reg, True)
    bound = (np.linalg.norm(g) + np.linalg.norm(gs)) / reg
    dist = np.linalg.norm(u - us)
    print("SVC-FIT %s std=%s %s: |u - u*| = %.3g, bound %.3g, status %s" % (IDS[i], standardization, path, dist, bound,
                                                                         model._solver_info["status"]))
    assert dist <= bound, (dist, bound)
    if model._solver_info["status"] == "converged (gradient)":
        # the optimiser's coordinates are sigma-scaled: theta = sigma w, whatever the penalty's scaling
        sig = X.astype(np.float64).std(0, ddof=1)
        tol_d = data_term_tol(Xd, y, u, 0.0, True, path)
        gq = g * q / sig
        assert np.all(np.abs(gq) <= 1e-6 * max(f, 1e-6) + tol_d[:-2] * q / sig), np.abs(gq).max()
    # predictions agree with the oracle's wherever its margin is larger than the coefficients can differ
    zs = Xd @ us
    safe = np.abs(zs) > np.linalg.norm(Xd, axis=1) * bound
    pred = model.transform(DataFrame.from_numpy(X, y)).to_numpy("prediction")
    assert safe.mean() > 0.9
    np.testing.assert_array_equal(pred[safe], (zs[safe] > 0).astype(np.float64))


def hinge_gap(i, path):
    X, y, reg, model = fit(i, "hinge", False)
    assert model._solver_info["path"] == path
    Xd = X.astype(np.float64)
    f = objective(Xd, y, np.asarray(model.coef_), 0.0, reg, False)[0]
    fs = objective(Xd, y, sk_optimum(i, False, False), 0.0, reg, False)[0]
    return (f - fs) / fs, model


@pytest.fixture
def cpu(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")


# ------------------------------------------------------------------------------------------
# fits, CPU path
@pytest.mark.parametrize("standardization", [False, True], ids=["raw", "std"])
@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_squared_hinge_matches_sklearn(cpu, i, standardization):
    check_squared_hinge(i, standardization, "torch-cpu")


@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_squared_hinge_with_intercept(cpu, i):
    X, y, reg, model = fit(i, "squared_hinge", False, fit_intercept=True)
    Xd = X.astype(np.float64)
    u, b = np.asarray(model.coef_), model.intercept
    f, g, gb = objective(Xd, y, u, b, reg, True)
    tol = data_term_tol(Xd, y, u, b, True, "torch-cpu")
    assert abs(model.objective - f) <= tol[-1] + 4 * U64 * abs(f), (model.objective, f)
    # f <= the fitIntercept=False optimum, up to what a fit stopped by the gradient test may be above
    # its own optimum: by convexity f(theta) - f(theta') <= grad f(theta) . (theta - theta') for
    # theta' = (u*, 0), and the stopping rule caps every entry of the gradient in the optimiser's
    # coordinates (theta_j = sigma_j w_j, the intercept unscaled) at tol max(f, tol), to which the
    # data term's own rounding adds its bound. The cap comes from tol, never from the fit's gradient.
    assert model._solver_info["status"] == "converged (gradient)", model._solver_info
    us = sk_optimum(i, True, False)
    fs = objective(Xd, y, us, 0.0, reg, True)[0]
    sig = Xd.std(0, ddof=1)
    gcap = 1e-6 * max(f, model.objective, 1e-6)
    cap = (gcap * (np.abs(sig * (u - us)).sum() + abs(b)) + tol[:-2] @ np.abs(u - us) + tol[-2] * abs(b))
    print("SVC-INTERCEPT %s: f - f*_nointercept = %.3g, cap %.3g" % (IDS[i], f - fs, cap))
    assert f <= fs + cap, (f, fs, cap)


@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_hinge_gap_cpu(cpu, i):
    g, model = hinge_gap(i, "torch-cpu")
    print("SVC-HINGE-GAP %s torch-cpu %.3g (%s, %d evaluations)" % (IDS[i], g, model._solver_info["status"],
                                                                   model._solver_info["n_evals"]))
    assert g <= 1e-4, g


# ------------------------------------------------------------------------------------------
# fits, GPU twin
@pytest.mark.gpu
@pytest.mark.parametrize("standardization", [False, True], ids=["raw", "std"])
@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_squared_hinge_matches_sklearn_gpu(gpu_device, i, standardization):
    check_squared_hinge(i, standardization, "fused_svc_f32")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(3), ids=IDS)
def test_hinge_gap_gpu(gpu_device, monkeypatch, i):
    g_dev, model = hinge_gap(i, "fused_svc_f32")
    monkeypatch.setenv("SRML_FORCE_CPU", "1")
    g_cpu, _ = hinge_gap(i, "torch-cpu")
    print("SVC-HINGE-GAP %s fused_svc_f32 %.3g vs torch-cpu %.3g (%s, %d evaluations)" % (
        IDS[i], g_dev, g_cpu, model._solver_info["status"], model._solver_info["n_evals"]))
    assert g_dev <= 3 * g_cpu, (g_dev, g_cpu)


@pytest.mark.gpu
def test_float64_inputs_select_f64_path(gpu_device):
    X, y = data(300, 8, 0.5)
    model = LinearSVC(regParam=0.01, loss="squared_hinge", float32_inputs=False).fit(DataFrame.from_numpy(X, y))
    assert model._solver_info["path"] == "lds_svc_f64" and model.dtype == "float64"


# ------------------------------------------------------------------------------------------
# API
def test_defaults_and_setters(cpu):
    est = LinearSVC()
    assert (est.getMaxIter(), est.getRegParam(), est.getTol(), est.getFitIntercept(), est.getStandardization(),
            est.getThreshold()) == (100, 0.0, 1e-6, True, True, 0.0)
    assert est.getOrDefault("aggregationDepth") == 2 and est.getOrDefault("maxBlockSizeInMB") == 0.0
    assert (est.getFeaturesCol(), est.getLabelCol(), est.getPredictionCol(), est.getRawPredictionCol()) == (
        "features", "label", "prediction", "rawPrediction")
    assert est.cuml_params["loss"] == "hinge" and est.cuml_params["C"] == 0.0 and est.cuml_params["penalty"] == "l2"
    est.setMaxIter(7).setRegParam(0.5).setTol(1e-3).setFitIntercept(False).setStandardization(False).setThreshold(0.25)
    assert (est.getMaxIter(), est.getRegParam(), est.getTol(), est.getFitIntercept(), est.getStandardization(),
            est.getThreshold()) == (7, 0.5, 1e-3, False, False, 0.25)
    cp = est.cuml_params
    assert (cp["max_iter"], cp["C"], cp["tol"], cp["fit_intercept"], cp["standardization"]) == (7, 2.0, 1e-3, False, False)
    assert LinearSVC(loss="squared_hinge").cuml_params["loss"] == "squared_hinge"
    c = est.copy({est.regParam: 0.25})
    assert c.getRegParam() == 0.25 and c.cuml_params["C"] == 4.0 and est.cuml_params["C"] == 2.0


def test_unsupported_params_raise(cpu):
    X, y = data(50, 3, 0.5)
    with pytest.raises(ValueError):
        LinearSVC(loss="logistic")
    with pytest.raises(ValueError):
        LinearSVC(weightCol="w").fit(DataFrame.from_numpy(X, y))
    for name in ("aggregationDepth", "maxBlockSizeInMB"):
        with pytest.raises(ValueError):
            LinearSVC(**{name: 3})
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        LinearSVC().fit(DataFrame.from_numpy(X, 2 * y))
    m = LinearSVC(maxIter=2).fit(DataFrame.from_numpy(X, y))
    with pytest.raises(NotImplementedError):
        m.evaluate(None)
    with pytest.raises(RuntimeError):
        m.summary
    assert not m.hasSummary
    with pytest.raises(ImportError):
        m.cpu()


def test_model_outputs_and_threshold(cpu):
    X, y = data(400, 6, 0.5)
    df = DataFrame.from_numpy(X, y)
    model = LinearSVC(regParam=0.01, loss="squared_hinge").fit(df)
    assert isinstance(model, LinearSVCModel) and model.numClasses == 2 and model.numFeatures == 6
    w, b = model.coefficients.toArray(), model.intercept
    z = X.astype(np.float64) @ w + b
    out = model.transform(df)
    raw = out.to_numpy("rawPrediction")
    np.testing.assert_allclose(raw[:, 1], z, rtol=0, atol=64 * U32 * (np.abs(X) @ np.abs(w) + abs(b)).max())
    np.testing.assert_array_equal(raw[:, 0], -raw[:, 1])
    np.testing.assert_array_equal(out.to_numpy("prediction"), (raw[:, 1] > 0).astype(np.float64))
    r0 = model.predictRaw(X[0]).toArray()
    assert r0[0] == -r0[1] and abs(r0[1] - z[0]) < 1e-12 and model.predict(X[0]) == float(z[0] > 0)
    thr = float(np.median(raw[:, 1])) + 0.5
    model.setThreshold(thr)
    assert model.getThreshold() == thr
    out2 = model.transform(df)
    np.testing.assert_array_equal(out2.to_numpy("rawPrediction"), raw)  # the threshold never moves rawPrediction
    np.testing.assert_array_equal(out2.to_numpy("prediction"), (raw[:, 1] > thr).astype(np.float64))
    assert out2.to_numpy("prediction").sum() < out.to_numpy("prediction").sum()
    assert model.predict(X[0]) == float(z[0] > thr)
    # an estimator's threshold reaches its model
    m2 = LinearSVC(regParam=0.01, loss="squared_hinge", threshold=thr).fit(df)
    np.testing.assert_array_equal(m2.transform(df).to_numpy("prediction"), out2.to_numpy("prediction"))


def test_sparse_input_matches_dense(cpu):
    import scipy.sparse as sp

    rng = np.random.default_rng(3)
    m, n, reg = 600, 30, 0.05
    A = sp.random(m, n, density=0.2, format="csr", random_state=rng, dtype=np.float64).astype(np.float32)
    Xd = np.asarray(A.todense(), dtype=np.float64)
    y = (Xd @ rng.standard_normal(n) > 0).astype(np.float64)
    kw = dict(regParam=reg, fitIntercept=False, standardization=False, loss="squared_hinge")
    md = LinearSVC(**kw).fit(DataFrame.from_numpy(Xd.astype(np.float32), y))
    ms = LinearSVC(enable_sparse_data_optim=True, **kw).fit(DataFrame.from_numpy(A, y, num_partitions=2))
    ud, us = np.asarray(md.coef_), np.asarray(ms.coef_)
    bound = (np.linalg.norm(objective(Xd, y, ud, 0.0, reg, True)[1])
             + np.linalg.norm(objective(Xd, y, us, 0.0, reg, True)[1])) / reg
    assert np.linalg.norm(ud - us) <= bound
    assert md._solver_info["status"] == ms._solver_info["status"] == "converged (gradient)"
    zs = ms.transform(DataFrame.from_numpy(A, y)).to_numpy("rawPrediction")[:, 1]
    np.testing.assert_allclose(zs, Xd @ us, atol=64 * U32 * (np.abs(Xd) @ np.abs(us)).max())


def test_constant_column_gets_zero(cpu):
    X, y = data(300, 5, 0.5)
    X[:, 2] = 3.0
    for std in (True, False):
        model = LinearSVC(regParam=0.01, standardization=std, loss="squared_hinge").fit(DataFrame.from_numpy(X, y))
        assert model.coef_[2] == 0.0 and np.all(np.asarray(model.coef_)[[0, 1, 3, 4]] != 0.0)


def test_save_load_round_trip(cpu, tmp_path):
    X, y = data(200, 5, 0.5)
    df = DataFrame.from_numpy(X, y)
    model = LinearSVC(regParam=0.01, loss="squared_hinge", threshold=0.125).fit(df)
    path = str(tmp_path / "svc")
    model.write().overwrite().save(path)
    m2 = LinearSVCModel.load(path)
    assert m2.coef_ == model.coef_ and m2.intercept_ == model.intercept_ and m2.getThreshold() == 0.125
    assert (m2.n_cols, m2.dtype, m2.num_iters, m2.objective) == (5, "float32", model.num_iters, model.objective)
    for col in ("prediction", "rawPrediction"):
        np.testing.assert_array_equal(m2.transform(df).to_numpy(col), model.transform(df).to_numpy(col))
    est = LinearSVC(maxIter=50, loss="squared_hinge")
    est.save(str(tmp_path / "svc_est"))
    e2 = LinearSVC.load(str(tmp_path / "svc_est"))
    assert e2.getMaxIter() == 50 and e2.cuml_params["loss"] == "squared_hinge"


def test_fit_multiple_equals_single_fits(cpu):
    X, y = data(500, 8, 0.5)
    df = DataFrame.from_numpy(X, y)
    est = LinearSVC(loss="squared_hinge")
    maps = [{est.regParam: r} for r in (0.001, 0.01, 0.1)]
    multi = [m for _, m in sorted(est.fitMultiple(df, maps), key=lambda t: t[0])]
    for pm, mm in zip(maps, multi):
        single = est.copy(pm).fit(df)
        assert mm.getRegParam() == pm[est.regParam]
        np.testing.assert_array_equal(np.asarray(mm.coef_), np.asarray(single.coef_))
        assert mm.intercept_ == single.intercept_


def test_cross_validator_single_pass(cpu):
    from spark_rapids_ml_nai_amd.tuning import CrossValidator, ParamGridBuilder

    X, y = data(500, 4, 0.3)
    df = DataFrame.from_numpy(X, y)
    est = LinearSVC(loss="squared_hinge")
    ev = MulticlassClassificationEvaluator(metricName="accuracy")
    assert est._supportsTransformEvaluate(ev) and est._enable_fit_multiple_in_single_pass()
    assert not est._supportsTransformEvaluate(MulticlassClassificationEvaluator(metricName="logLoss"))
    grid = ParamGridBuilder().addGrid(est.regParam, [0.001, 0.1]).build()
    cvm = CrossValidator(estimator=est, estimatorParamMaps=grid, evaluator=ev, numFolds=2, seed=1).fit(df)
    assert min(cvm.avgMetrics) > 0.85
    models = [m for _, m in sorted(est.fitMultiple(df, grid), key=lambda t: t[0])]
    fast = models[0]._combine(models)._transformEvaluate(df, ev)
    np.testing.assert_allclose(fast, [ev.evaluate(m.transform(df)) for m in models], rtol=1e-12)


# ------------------------------------------------------------------------------------------
# two gloo ranks against one
def _two_rank_fits(loss, fit_intercept=False, standardization=False):
    m, n, reg, noise = DATASETS[1]
    X, y = data(m, n, noise)
    df = DataFrame.from_numpy(X, y, num_partitions=2)
    kw = dict(regParam=reg, fitIntercept=fit_intercept, standardization=standardization, loss=loss)
    return X, y, reg, LinearSVC(num_workers=1, **kw).fit(df), LinearSVC(num_workers=2, **kw).fit(df)


@pytest.mark.dist
def test_two_ranks_match_one_rank(cpu):
    X, y, reg, a, b = _two_rank_fits("squared_hinge")
    Xd = X.astype(np.float64)
    ua, ub = np.asarray(a.coef_), np.asarray(b.coef_)
    bound = (np.linalg.norm(objective(Xd, y, ua, 0.0, reg, True)[1])
             + np.linalg.norm(objective(Xd, y, ub, 0.0, reg, True)[1])) / reg
    assert np.linalg.norm(ua - ub) <= bound, (np.linalg.norm(ua - ub), bound)
    assert a._solver_info["status"] == b._solver_info["status"] == "converged (gradient)"


@pytest.mark.dist
def test_two_ranks_bad_labels_raise_everywhere(cpu):
    X, y = data(200, 4, 0.5)
    y[150:] *= 2  # only the second rank's shard holds a label 2
    with pytest.raises(Exception, match="labels must be 0 or 1"):
        LinearSVC(num_workers=2).fit(DataFrame.from_numpy(X, y, num_partitions=2))


@pytest.mark.dist
@pytest.mark.parametrize("loss,fit_intercept,standardization", [("squared_hinge", False, False),
                                                                ("squared_hinge", True, True), ("hinge", True, False)])
def test_two_ranks_deterministic_bit_equal(cpu, monkeypatch, loss, fit_intercept, standardization):
    monkeypatch.setenv("SRML_DETERMINISTIC", "1")
    X, y, reg, a, b = _two_rank_fits(loss, fit_intercept, standardization)
    ua, ub = np.asarray(a.coef_), np.asarray(b.coef_)
    assert np.array_equal(ua, ub), "max |w_2 - w_1| = %.3g" % np.abs(ua - ub).max()
    assert a.intercept_ == b.intercept_ and a.objective == b.objective and a.num_iters == b.num_iters
    if loss == "squared_hinge" and not fit_intercept:  # and it is still the same optimum
        us = sk_optimum(1, True, False)
        Xd = X.astype(np.float64)
        bound = (np.linalg.norm(objective(Xd, y, ua, 0.0, reg, True)[1])
                 + np.linalg.norm(objective(Xd, y, us, 0.0, reg, True)[1])) / reg
        assert np.linalg.norm(ua - us) <= bound
