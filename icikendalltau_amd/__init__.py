"""icikendalltau_amd -- MI355X-native all-pairs ICI-Kendall-tau (drop-in for ICIKendallTau's
ici_kendalltau() / ici_kt() path).  See DESIGN.md and include/icikt.h."""
from ._lib import Context, IciktError, build, default_context, device_count  # noqa: F401
from .api import (HipEngine, IciKtResult, PreparedReference, prepare_reference, calculate_matrix_medians, cor_fast, ici_kendalltau, ici_kendalltau_anosim, ici_kendalltau_class_matrix, ici_kendalltau_cross, ici_kendalltau_edges,  # noqa: F401
                  ici_kendalltau_hclust, ici_kendalltau_mantel, mantel_permutations, mantel_statistic, ici_kendalltau_medians, ici_kendalltau_mst, ici_kendalltau_padjust, ici_kendalltau_pcoa, ici_kendalltau_permanova, ici_kendalltau_permdisp, ici_kendalltau_quantiles, ici_kendalltau_significant, ici_kendalltau_topk, ici_kt, ici_kt_counts, kt_fast, pairwise_completeness, rank_order_data, setup_comparisons,
                  setup_missing_matrix, test_left_censorship)

from .formats import cor_matrix_2_long_df, cross_topk_to_csr, edges_to_coo, hclust_cut, hclust_to_linkage, long_df_2_cor_matrix, mst_cut, mst_to_linkage, read_r_data, read_r_matrix, topk_to_csr  # noqa: F401

__version__ = "0.1.0"
