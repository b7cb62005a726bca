from .baselines import (  # noqa: F401
    ArticleFeatureBaseline, InviewEstimateBaseline, PopularityIndex, RecentPopularity, lexicographic_scores, window_counts_host,
)
