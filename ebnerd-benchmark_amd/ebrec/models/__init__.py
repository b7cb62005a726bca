from .baselines import (  # noqa: F401
    ArticleFeatureBaseline, ContentSimilarity, InviewEstimateBaseline, PopularityIndex, RecentPopularity, content_centroid_scores_host,
    content_nearest_scores_host, content_profiles_host, lexicographic_scores, window_counts_host,
)
