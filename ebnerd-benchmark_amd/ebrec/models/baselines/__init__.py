from .popularity import (  # noqa: F401
    ArticleFeatureBaseline, InviewEstimateBaseline, PopularityIndex, RecentPopularity, WindowCounts, lexicographic_scores,
    window_counts_host,
)
