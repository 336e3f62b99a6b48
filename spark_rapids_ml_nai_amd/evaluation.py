"""``pyspark.ml.evaluation``-compatible evaluators for the Spark-free data plane.

``RegressionEvaluator`` (rmse, mse, r2, mae, var), ``MulticlassClassificationEvaluator``
(the 14 Spark metrics), ``BinaryClassificationEvaluator`` (areaUnderROC / areaUnderPR) and
``ClusteringEvaluator`` (silhouette, squaredEuclidean / cosine) evaluate a transformed DataFrame;
the CrossValidator fast path skips the transformed frame and merges per-partition statistics
computed on the device (``metrics/``).
When pyspark is installed its evaluators are accepted as well (same getters).
"""
from __future__ import annotations

from typing import Any, List, Optional, Union

import numpy as np

from .core.dataframe import DataFrame, as_dataframe, vector_column_is_sparse, vector_column_to_csr
from .core.params import HasEnableSparseDataOptim, HasFeaturesCol, HasFeaturesCols, HasLabelCol, HasPredictionCol, \
    HasProbabilityCol, HasRawPredictionCol, Param, Params, TypeConverters, keyword_only
from .metrics import ClassificationSummary, MulticlassMetrics, RegressionMetrics, RegressionSummary, binary_aupr, \
    binary_auc


def _local(dataset: Any, cols: list) -> DataFrame:
    """The evaluated columns as a local DataFrame; a Spark DataFrame is reduced to those columns
    and brought to the driver through Arrow (``toArrow`` on Spark 4, ``toPandas`` before)."""
    from .parallel.spark import is_spark_dataframe

    if is_spark_dataframe(dataset):
        sel = dataset.select(*[c for c in cols if c in dataset.columns])
        if hasattr(sel, "toArrow"):
            return DataFrame([sel.toArrow()])
        return as_dataframe(sel.toPandas())[0]
    return as_dataframe(dataset)[0]


class Evaluator(Params):
    def evaluate(self, dataset: Any, params: Optional[dict] = None) -> float:
        if params:
            return self.copy(params)._evaluate(dataset)
        return self._evaluate(dataset)

    def _evaluate(self, dataset: Any) -> float:
        raise NotImplementedError

    def isLargerBetter(self) -> bool:
        return True

    def getMetricName(self) -> str:
        return self.getOrDefault("metricName")

    def setMetricName(self, value: str) -> "Evaluator":
        return self._set(metricName=value)

    def setLabelCol(self, value: str) -> "Evaluator":
        return self._set(labelCol=value)

    def setPredictionCol(self, value: str) -> "Evaluator":
        return self._set(predictionCol=value)


class RegressionEvaluator(Evaluator, HasLabelCol, HasPredictionCol):
    metricName = Param(Params._dummy(), "metricName", "metric name in evaluation - one of: rmse, mse, r2, mae, var",
                       typeConverter=TypeConverters.toString)
    throughOrigin = Param(Params._dummy(), "throughOrigin", "whether the regression is through the origin.",
                          typeConverter=TypeConverters.toBoolean)
    weightCol = Param(Params._dummy(), "weightCol", "weight column name.", typeConverter=TypeConverters.toString)

    @keyword_only
    def __init__(self, *, predictionCol: str = "prediction", labelCol: str = "label", metricName: str = "rmse",
                 weightCol: Optional[str] = None, throughOrigin: bool = False) -> None:
        super().__init__()
        self._setDefault(metricName="rmse", throughOrigin=False, labelCol="label", predictionCol="prediction")
        self._set(**{k: v for k, v in self._input_kwargs.items() if v is not None})

    def getThroughOrigin(self) -> bool:
        return self.getOrDefault("throughOrigin")

    def isLargerBetter(self) -> bool:
        return self.getMetricName() in ("r2", "var")

    def _evaluate(self, dataset: Any) -> float:
        df = _local(dataset, [self.getOrDefault("labelCol"), self.getOrDefault("predictionCol")])
        y = df.to_numpy(self.getOrDefault("labelCol"), np.float64)
        p = df.to_numpy(self.getOrDefault("predictionCol"), np.float64)
        return RegressionMetrics(RegressionSummary.from_arrays(y, p)).evaluate(self)


class MulticlassClassificationEvaluator(Evaluator, HasLabelCol, HasPredictionCol, HasProbabilityCol):
    metricName = Param(Params._dummy(), "metricName", "metric name in evaluation", typeConverter=TypeConverters.toString)
    metricLabel = Param(Params._dummy(), "metricLabel", "The class whose metric will be computed",
                        typeConverter=TypeConverters.toFloat)
    beta = Param(Params._dummy(), "beta", "The beta value used in weightedFMeasure|fMeasureByLabel",
                 typeConverter=TypeConverters.toFloat)
    eps = Param(Params._dummy(), "eps", "log-loss clipping epsilon", typeConverter=TypeConverters.toFloat)
    weightCol = Param(Params._dummy(), "weightCol", "weight column name.", typeConverter=TypeConverters.toString)

    @keyword_only
    def __init__(self, *, predictionCol: str = "prediction", labelCol: str = "label", metricName: str = "f1",
                 weightCol: Optional[str] = None, metricLabel: float = 0.0, beta: float = 1.0,
                 probabilityCol: str = "probability", eps: float = 1e-15) -> None:
        super().__init__()
        self._setDefault(metricName="f1", metricLabel=0.0, beta=1.0, eps=1e-15, labelCol="label",
                         predictionCol="prediction", probabilityCol="probability")
        self._set(**{k: v for k, v in self._input_kwargs.items() if v is not None})

    def getMetricLabel(self) -> float:
        return self.getOrDefault("metricLabel")

    def getBeta(self) -> float:
        return self.getOrDefault("beta")

    def getEps(self) -> float:
        return self.getOrDefault("eps")

    def isLargerBetter(self) -> bool:
        return self.getMetricName() not in ("weightedFalsePositiveRate", "falsePositiveRateByLabel", "hammingLoss",
                                            "logLoss")

    def _evaluate(self, dataset: Any) -> float:
        df = _local(dataset, [self.getOrDefault(c) for c in ("labelCol", "predictionCol", "probabilityCol")])
        y = df.to_numpy(self.getOrDefault("labelCol"), np.float64)
        p = df.to_numpy(self.getOrDefault("predictionCol"), np.float64)
        prob = None
        if self.getMetricName() == "logLoss":
            prob = df.to_numpy(self.getOrDefault("probabilityCol"), np.float64)
        return MulticlassMetrics(ClassificationSummary.from_arrays(y, p, prob, self.getEps())).evaluate(self)


class BinaryClassificationEvaluator(Evaluator, HasLabelCol, HasRawPredictionCol):
    metricName = Param(Params._dummy(), "metricName", "areaUnderROC|areaUnderPR", typeConverter=TypeConverters.toString)
    numBins = Param(Params._dummy(), "numBins", "number of bins for the curves", typeConverter=TypeConverters.toInt)

    @keyword_only
    def __init__(self, *, rawPredictionCol: str = "rawPrediction", labelCol: str = "label",
                 metricName: str = "areaUnderROC", weightCol: Optional[str] = None, numBins: int = 1000) -> None:
        super().__init__()
        self._setDefault(metricName="areaUnderROC", numBins=1000, labelCol="label", rawPredictionCol="rawPrediction")
        self._set(**{k: v for k, v in self._input_kwargs.items() if v is not None and k != "weightCol"})

    def _evaluate(self, dataset: Any) -> float:
        df = _local(dataset, [self.getOrDefault("labelCol"), self.getOrDefault("rawPredictionCol")])
        y = df.to_numpy(self.getOrDefault("labelCol"), np.float64)
        rc = self.getOrDefault("rawPredictionCol")
        raw = df.to_numpy(rc, np.float64)
        score = raw[:, -1] if raw.ndim == 2 else raw
        if self.getMetricName() == "areaUnderPR":
            return binary_aupr(y, score)
        return binary_auc(y, score)


class ClusteringEvaluator(Evaluator, HasPredictionCol, HasFeaturesCol, HasFeaturesCols, HasEnableSparseDataOptim):
    """Silhouette of a clustering (``pyspark.ml.evaluation.ClusteringEvaluator``): Spark's closed
    form, every row scored against the k cluster summaries on the fused MFMA kernel.
    ``enable_sparse_data_optim=True`` (or ``None`` and a sparse first row) keeps a vector column CSR
    and scores it on the CSR kernels without densifying; the default ``False`` densifies as before.
    Array and multi-column features ignore the flag."""
    metricName = Param(Params._dummy(), "metricName", "metric name in evaluation (silhouette)",
                       typeConverter=TypeConverters.toString)
    distanceMeasure = Param(Params._dummy(), "distanceMeasure", "The distance measure. Supported options: "
                            "'squaredEuclidean' and 'cosine'.", typeConverter=TypeConverters.toString)
    weightCol = Param(Params._dummy(), "weightCol", "weight column name.", typeConverter=TypeConverters.toString)

    @keyword_only
    def __init__(self, *, predictionCol: str = "prediction", featuresCol: Union[str, List[str]] = "features",
                 metricName: str = "silhouette", distanceMeasure: str = "squaredEuclidean",
                 weightCol: Optional[str] = None, enable_sparse_data_optim: Optional[bool] = False) -> None:
        super().__init__()
        self._setDefault(metricName="silhouette", distanceMeasure="squaredEuclidean", predictionCol="prediction",
                         featuresCol="features", enable_sparse_data_optim=False)
        kw = {k: v for k, v in self._input_kwargs.items() if v is not None}
        if "enable_sparse_data_optim" in self._input_kwargs:  # None is a value here: the first row decides
            self._set(enable_sparse_data_optim=self._input_kwargs["enable_sparse_data_optim"])
            kw.pop("enable_sparse_data_optim", None)
        fc = kw.pop("featuresCol", None)
        self._set(**kw)
        if fc is not None:
            self.setFeaturesCol(fc)
        self._check()

    def _check(self) -> None:
        from .ops import SILHOUETTE_MEASURES

        if self.getMetricName() != "silhouette":
            raise ValueError("ClusteringEvaluator: metricName must be 'silhouette', got %r" % self.getMetricName())
        if self.getDistanceMeasure() not in SILHOUETTE_MEASURES:
            raise ValueError("ClusteringEvaluator: distanceMeasure must be one of %s, got %r"
                             % (SILHOUETTE_MEASURES, self.getDistanceMeasure()))

    def getDistanceMeasure(self) -> str:
        return self.getOrDefault("distanceMeasure")

    def setDistanceMeasure(self, value: str) -> "ClusteringEvaluator":
        return self._set(distanceMeasure=value)

    def getWeightCol(self) -> Optional[str]:
        return self.getOrDefault("weightCol") if self.isDefined("weightCol") else None

    def setWeightCol(self, value: str) -> "ClusteringEvaluator":
        return self._set(weightCol=value)

    def setFeaturesCol(self, value: Union[str, List[str]]) -> "ClusteringEvaluator":
        if isinstance(value, str):
            self.clear(self.getParam("featuresCols"))
            return self._set(featuresCol=value)
        return self._set(featuresCols=list(value))

    def _use_sparse(self, df: DataFrame, col: Optional[str]) -> bool:
        if col is None or not df.is_vector(col):
            return False
        flag = self.getOrDefault("enable_sparse_data_optim")
        return vector_column_is_sparse(df.column(col)) if flag is None else bool(flag)

    def _evaluate(self, dataset: Any) -> float:
        from .core.base import _dense_from_df
        from .models.silhouette import silhouette_score
        from .parallel.context import local_device

        self._check()
        cols = self.getOrDefault("featuresCols") if self.isDefined("featuresCols") else None
        col = None if cols else self.getOrDefault("featuresCol")
        pc, wc = self.getOrDefault("predictionCol"), self.getWeightCol()
        df = _local(dataset, (cols or [col]) + [pc] + ([wc] if wc else []))
        sparse = self._use_sparse(df, col)  # one decision for every partition
        parts = []
        for t in df.partitions:
            if t.num_rows == 0:
                continue
            p = DataFrame([t])
            X = vector_column_to_csr(p.column(col), np.float32) if sparse else _dense_from_df(p, col, cols, np.float32)
            parts.append((X, p.to_numpy(pc, np.float64),
                          p.to_numpy(wc, np.float64) if wc else None))
        return silhouette_score(parts, self.getDistanceMeasure(), local_device())
