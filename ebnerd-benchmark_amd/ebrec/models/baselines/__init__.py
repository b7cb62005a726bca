from .als import ImplicitALS, als_loss_host, als_partials_host, als_scores_host, als_solve_host  # noqa: F401
from .content import (  # noqa: F401
    ContentSimilarity, content_centroid_scores_host, content_nearest_scores_host, content_profiles_host, history_weight_values,
    unit_rows_host,
)
from .covisit import (  # noqa: F401
    CoVisitation, CoVisitMatrix, covisit_matrix_host, covisit_pair_keys_host, covisit_scores_host, covisit_target_rank_host,
    covisit_topk_host, covisit_transpose_host, covisit_values_host,
)
from .ease import (EASE, ease_gram_host, ease_invert_host, ease_scores_host, ease_system_host, ease_target_rank_host, ease_topk_host,  # noqa: F401
                   ease_weights_host)
from .knn import (HistoryKNN, KNNIndex, knn_index_host, knn_neighbours_host, knn_scores_host, knn_target_rank_host,  # noqa: F401
                  knn_topk_host)
from ._topn import TopN, dense_target_rank_host, dense_topk_host  # noqa: F401
from .popularity import (  # noqa: F401
    ArticleFeatureBaseline, InviewEstimateBaseline, PopularityIndex, RecentPopularity, WindowCounts, lexicographic_scores,
    window_counts_host,
)
