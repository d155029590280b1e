"""bsms_gnn_amd: MI355X-native engine for the BSMS-GNN multi-level message-passing path.

Host-side mirror of the reference's `src/ops` + `src/models` interface over the C ABI of
libbsms_hip.so (include/bsms_hip.h).  Import name: `bsms_gnn_amd` (directory: `bsms-gnn_amd/`)."""
from . import _abi  # noqa: F401
from .graph import LevelData, LevelPlan, MeshBank, clear_plan_cache, collate_variable_meshes, concat_plans, plan_for  # noqa: F401
from .model import BSMS_Simulator, Normalizer, masked_rmse  # noqa: F401
from .objective import Objective, edge_difference_loss, edge_difference_sums, masked_loss  # noqa: F401
from .ops import BSGMP, GMP, MLP, InferenceSession, Unpool, WeightedEdgeConv, degree, edge_diff_bwd, edge_diff_sums, error_sums, moment_fold, moment_sums, scatter_sum  # noqa: F401
from .eval import cell_error_mean_std, divergence_rms, edge_error_mean_std, equivariance_error, error_mean_std  # noqa: F401
from .databank import Augment, Moments, TrajectoryBank, epoch_picks, fit_normalizers, transform_rows  # noqa: F401
from .dp import DataParallel, GradBuckets, global_masked_rmse  # noqa: F401
from .hierarchy import BistrideMultiLayerGraph, lumped_node_measure, to_flat_edge  # noqa: F401
from .rollout import RolloutErrors, rank_slice, rollout_bank, rollout_batch, rollout_dataset, rollout_errors, rollout_one_traj, rollout_rmse  # noqa: F401
from .sample import MeshSampler, rollout_frames, write_png  # noqa: F401
from .diffop import MeshGradient, cell_gradient_loss  # noqa: F401
from .step import FusedStep, input_gradient  # noqa: F401
from .trainer import DevicePrefetcher, FusedAdamW, Trainer, WarmupCosineDecay, param_groups, segment_table  # noqa: F401

__version__ = "0.1.0"
