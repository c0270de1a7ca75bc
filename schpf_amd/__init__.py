"""schpf_amd -- MI355X-native engine for the scHPF CAVI hot path.

Host side: the reference's Python API (scHPF estimator, HPF_Gamma, loss functions,
the hpf_numba operator names) re-implemented over a C-ABI HIP library
(include/schpf_hip.h, schpf_amd/csrc/).  There is no CPU compute path.
"""
from ._version import __version__
from . import hpf_hip, loss, preprocessing
from .engine import DeviceCAVI
from .scHPF_ import HPF_Gamma, scHPF, load_model, save_model, combine_across_cells
from .trials import run_trials, run_trials_pool
from .thinning import thin_counts
from .neighbors import knn, knn_graph, knn_connectivities, louvain, modularity
from .topology import connected_components, cluster_graph, absorb_small, paga
from .paths import geodesic_distances, pseudotime, farthest_landmarks, landmark_isomap
from .markers import rank_sums, rank_genes_groups, pair_rank_sums, rank_genes_pairs
from .doublets import simulate_doublets, doublet_scores
from .qc import qc_metrics, submatrix, filter_counts
from .aggregate import group_stats, pseudobulk, group_codes
from .variable_genes import residual_variance, highly_variable_genes
from .gene_major import GeneMajor, gene_major

# make the pickle module path of the classes (schpf.scHPF_) resolvable
import schpf.scHPF_  # noqa: E402,F401

__all__ = ["__version__", "hpf_hip", "loss", "preprocessing", "DeviceCAVI", "HPF_Gamma", "scHPF", "load_model",
           "save_model", "combine_across_cells", "run_trials", "run_trials_pool", "thin_counts", "knn", "knn_graph",
           "knn_connectivities", "louvain", "modularity", "rank_sums", "rank_genes_groups", "pair_rank_sums", "rank_genes_pairs", "simulate_doublets",
           "doublet_scores", "qc_metrics", "submatrix", "filter_counts", "group_stats", "pseudobulk", "group_codes",
           "connected_components", "cluster_graph", "absorb_small", "paga", "geodesic_distances", "pseudotime",
           "farthest_landmarks", "landmark_isomap", "residual_variance", "highly_variable_genes", "GeneMajor",
           "gene_major"]
