"""ClusteringEvaluator / ops.silhouette (fp64 torch path) against the direct O(m^2) definition.

Tolerance: both sides are fp64; the closed form cancels at most (||v|| + ||m|| + sqrt t)^2 / max(a, b),
below 1e3 for the blobs here, so 1e-10 leaves three digits over 1e3 * n * 2^-53."""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.evaluation import ClusteringEvaluator

TOL = 1e-10
MEASURES = ("squaredEuclidean", "cosine")


def oracle(X, lab, w=None, measure="squaredEuclidean"):
    """(s, a, b) per row from the pairwise distances: weighted means per cluster, self excluded by N - w."""
    X = np.asarray(X, np.float64)
    w = np.ones(len(X)) if w is None else np.asarray(w, np.float64)
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True) if measure == "cosine" else X
    D = 1.0 - Xn @ Xn.T if measure == "cosine" else ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    ids, rows = np.unique(lab[w > 0]), np.arange(len(X))
    W = np.stack([w * (lab == c) for c in ids], 1)
    N, own = W.sum(0), np.searchsorted(ids, lab).clip(max=len(ids) - 1)
    tot = D @ W
    with np.errstate(divide="ignore", invalid="ignore"):
        a = tot[rows, own] / (N[own] - w)
        oth = tot / N
        oth[rows, own] = np.inf
        b = oth.min(1)
        s = np.where(a < b, 1 - a / b, np.where(a > b, b / a - 1, 0.0))
    s[(N[own] <= w) | (w == 0)] = 0.0
    return s, a, b


@pytest.fixture(autouse=True)
def _cpu(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")


@pytest.fixture(scope="module")
def blobs():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 3, 300)
    X = (rng.standard_normal((300, 5)) + 8.0 * rng.standard_normal((3, 5))[lab]).astype(np.float32)
    w = rng.uniform(0.5, 2.0, 300)
    w[17] = 0.0
    lab[5], lab[17] = 3, 4  # a singleton; the weightless row's cluster vanishes with it
    return X, lab, w, np.array([0.0, 5.0, 7.0, 11.0, -2.0])[lab]  # non-contiguous prediction values


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("weighted", (False, True))
def test_op_and_evaluator_match_definition(blobs, measure, weighted):
    X, lab, w, pred = blobs
    w = w if weighted else None
    s, _, _ = oracle(X, lab, w, measure)
    ww = np.ones(len(X)) if w is None else w
    score = (ww * s).sum() / ww.sum()
    sws, sw, rows = ops.silhouette(torch.from_numpy(X), torch.from_numpy(lab), 5,
                                   None if w is None else torch.from_numpy(w), measure, rows_out=True)
    assert abs(float(sw) - ww.sum()) <= TOL * ww.sum()
    assert abs(float(sws) / float(sw) - score) <= TOL
    assert np.abs(rows.numpy() - s).max() <= 2.0 ** -24 + TOL  # the rows come back as fp32
    assert rows[5] == 0 and rows[17] == 0
    df = DataFrame.from_numpy(X, extra={"prediction": pred, "w": ww})
    ev = ClusteringEvaluator(distanceMeasure=measure, weightCol="w" if weighted else None)
    assert ev.isLargerBetter() and ev.getMetricName() == "silhouette" and ev.getDistanceMeasure() == measure
    one = ev.evaluate(df)
    assert abs(one - score) <= TOL
    three = ev.evaluate(DataFrame.from_numpy(X, extra={"prediction": pred, "w": ww}, num_partitions=3))
    assert abs(three - one) <= TOL
    cols = DataFrame.from_pandas(__import__("pandas").DataFrame(
        {**{"f%d" % j: X[:, j] for j in range(5)}, "prediction": pred, "w": ww}))
    assert abs(ev.copy().setFeaturesCol(["f%d" % j for j in range(5)]).evaluate(cols) - score) <= TOL


def test_ties_duplicates_and_singleton_score_zero():
    # (0,0): a = b = 4; the four copies of (8,8) split over two clusters: a = b = 0; (5,5) is alone
    X = np.array([[0, 0], [2, 0], [0, 2], [0, -2], [8, 8], [8, 8], [8, 8], [8, 8], [5, 5]], np.float32)
    lab = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4])
    s, _, _ = oracle(X, lab)
    sws, sw, rows = ops.silhouette(torch.from_numpy(X), torch.from_numpy(lab), 5, rows_out=True)
    assert np.abs(rows.numpy() - s).max() <= 2.0 ** -24
    assert (rows[[0, 4, 5, 6, 7, 8]] == 0).all() and float(sw) == 9.0
    assert abs(float(sws) - s.sum()) <= TOL


def test_errors():
    X = np.random.default_rng(0).standard_normal((6, 2)).astype(np.float32)
    lab = np.array([0.0, 0, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="greater than one"):
        ClusteringEvaluator().evaluate(DataFrame.from_numpy(X, extra={"prediction": np.zeros(6)}))
    Z = X.copy()
    Z[2] = 0
    with pytest.raises(ValueError, match="zero"):
        ClusteringEvaluator(distanceMeasure="cosine").evaluate(DataFrame.from_numpy(Z, extra={"prediction": lab}))
    for bad in (-1.0, np.inf):
        w = np.ones(6)
        w[1] = bad
        with pytest.raises(ValueError, match="weights"):
            ClusteringEvaluator(weightCol="w").evaluate(DataFrame.from_numpy(X, extra={"prediction": lab, "w": w}))
    with pytest.raises(ValueError):
        ClusteringEvaluator(metricName="dunn")
    with pytest.raises(ValueError):
        ClusteringEvaluator(distanceMeasure="euclidean")


def test_kmeans_transform_evaluate():
    from spark_rapids_ml_nai_amd.clustering import KMeans

    rng = np.random.default_rng(10)
    X = np.concatenate([rng.standard_normal((60, 4)) + 8 * i for i in range(3)]).astype(np.float32)
    df = DataFrame.from_numpy(X)
    out = KMeans(k=3, seed=1).fit(df).transform(df)
    s, _, _ = oracle(X, out.to_numpy("prediction").astype(np.int64))
    assert abs(ClusteringEvaluator().evaluate(out) - s.mean()) <= TOL
