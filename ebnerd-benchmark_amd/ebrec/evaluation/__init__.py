from .metrics_protocols import (  # noqa: F401
    AccuracyScore, AucScore, F1Score, LogLossScore, MetricEvaluator, MrrScore, NdcgScore, RootMeanSquaredError,
)
from .beyond_accuracy import Calibration, Coverage, Distribution, IntralistDiversity, Novelty, Serendipity  # noqa: F401
from .device_metrics import DeviceMetricEvaluator, RaggedLists  # noqa: F401
from .rerank import DPP, MMR, Calibrated, calibrated_rerank, dpp_rerank, history_distribution, mmr_rerank  # noqa: F401
from .freshness import Freshness  # noqa: F401
from .catalogue_ranks import rank_metrics  # noqa: F401
