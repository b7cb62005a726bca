from .baselines import (  # noqa: F401
    ArticleFeatureBaseline, ContentSimilarity, CoVisitation, HistoryKNN, ImplicitALS, InviewEstimateBaseline, PopularityIndex, RecentPopularity,
    als_loss_host, als_partials_host, als_scores_host, als_solve_host, content_centroid_scores_host, content_nearest_scores_host, content_profiles_host, covisit_matrix_host, covisit_pair_keys_host,
    covisit_scores_host, covisit_target_rank_host, covisit_topk_host, covisit_transpose_host, covisit_values_host, dense_target_rank_host,
    dense_topk_host, EASE, ease_gram_host, ease_invert_host, ease_scores_host, ease_system_host, ease_target_rank_host, ease_topk_host, ease_weights_host, knn_index_host, knn_neighbours_host, knn_scores_host, knn_target_rank_host, knn_topk_host, lexicographic_scores, window_counts_host,
)
from .ensemble import (  # noqa: F401
    RankFusion, ScoreBlend, blend_combine_host, blend_features_host, blend_sums_host,
)
