from .metrics_protocols import (  # noqa: F401
    AccuracyScore, AucScore, F1Score, LogLossScore, MetricEvaluator, MrrScore, NdcgScore, RootMeanSquaredError,
)
from .beyond_accuracy import Calibration, Coverage, Distribution, IntralistDiversity, Novelty, Serendipity  # noqa: F401
from .device_metrics import DeviceMetricEvaluator, RaggedLists  # noqa: F401
from .rerank import DPP, MMR, Calibrated, calibrated_rerank, dpp_rerank, history_distribution, mmr_rerank  # noqa: F401
from .freshness import Freshness  # noqa: F401
from .catalogue_ranks import bootstrap_rank_metrics, rank_metrics, rank_values  # noqa: F401
from .bootstrap import (  # noqa: F401
    BootstrapResult, PairedBootstrapResult, bootstrap_evaluator, bootstrap_means, paired_bootstrap, poisson_bootstrap_sums,
)
