"""sdfest_amd -- MI355X-native implementation of sdfest's render-and-compare hot path.

Public surface mirrors the reference's ``sdfest.differentiable_renderer``
(``Camera``, ``render_depth_gpu``) so that ``SDFPipeline.render`` can bind to it
unchanged; see INTEGRATION.md.
"""
from .differentiable_renderer import (BatchRenderPlan, Camera, SDFRendererFunctionGPU,
                                      render_depth_batch, render_depth_l1_batch,
                                      render_depth_gpu)

from .losses import nn_loss, pc_loss, pc_loss_batch, point_constraint_loss
from .vae import SDFDecoder, SDFEncoder, SDFVAE
from .train import SDFVAETrainer
from .pipeline import FusedRenderAndCompare, RenderAndCompare
from .init_network import NoDepthError, SDFPoseNet, nn_init
from .init_train import SDFPoseNetTrainer
from .mesh import Mesh, draw_depth_geometry, extract_mesh, render_mesh_depth, sample_points, visible_mask
from .boxes import box_iou, sdf_bounds
from .ap import average_precision, match_detections, pair_table, pose_pair_errors
from .metrics import (accuracy_thresh, completeness_thresh, correct_thresh, evaluate_metrics, extent, iou_3d,
                      mean_accuracy, mean_average_precision, mean_completeness, reconstruction_fscore, reconstruction_metrics,
                      symmetric_chamfer)
from .simple_setup import SDFPipeline
from .sdf_utils import mesh_to_sdf
from .evaluation import evaluate_annotated, evaluate_mesh, evaluate_meshes, generate_views, vae_reconstruction
from .so3grid import SO3Grid
from . import nocs_utils, pointset_utils
from .nocs_dataset import NOCSDataset
from .redwood_dataset import AnnotatedRedwoodDataset
from .uncertainty import (PoseUncertainty, ShapePoseUncertainty, combine_information, joint_tangent_information, pc_information,
                          pose_covariance, render_information, sdf_std, shape_pose_covariance, tangent_information, tangent_map)
from .lm import LMRefiner, LMReport, lm_step
from .visualization import depth_range, render_normals, shade_frames, trajectory_frames, write_animation, write_frames

__all__ = ["render_normals", "depth_range", "shade_frames", "trajectory_frames", "write_frames", "write_animation", "pc_information", "combine_information", "lm_step", "LMRefiner", "LMReport", "ShapePoseUncertainty", "joint_tangent_information", "shape_pose_covariance", "sdf_std", "mean_average_precision", "average_precision", "match_detections", "pair_table", "pose_pair_errors", "box_iou", "sdf_bounds", "iou_3d", "PoseUncertainty", "pose_covariance", "render_information", "tangent_information", "tangent_map",
           "AnnotatedRedwoodDataset", "visible_mask", "evaluate_annotated", "NOCSDataset", "nocs_utils", "pointset_utils", "SDFPipeline", "generate_views", "evaluate_mesh", "evaluate_meshes", "vae_reconstruction", "mesh_to_sdf", "Mesh", "extract_mesh", "sample_points", "render_mesh_depth", "draw_depth_geometry", "mean_accuracy", "mean_completeness", "symmetric_chamfer", "accuracy_thresh", "completeness_thresh", "reconstruction_fscore", "extent", "correct_thresh", "reconstruction_metrics", "evaluate_metrics", "NoDepthError", "RenderAndCompare", "FusedRenderAndCompare", "SDFPoseNet", "nn_init", "SO3Grid", "SDFDecoder", "SDFEncoder", "SDFVAE", "SDFVAETrainer", "SDFPoseNetTrainer", "pc_loss", "pc_loss_batch", "nn_loss", "point_constraint_loss", "BatchRenderPlan", "Camera", "SDFRendererFunctionGPU", "render_depth_gpu", "render_depth_batch", "render_depth_l1_batch"]
