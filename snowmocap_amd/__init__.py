"""snowmocap_amd -- MI355X-native multi-view triangulation core behind SnowMocap's
`snowvision.triangulation` / `camera.CameraGroup` API.

Importing the package does not load the HIP library; the first call that needs it does, and
fails loudly if libsnowtri.so was not built or no GPU is visible (there is no CPU fallback).
"""
from .camera import Camera, CameraGroup
from .triangulation import (Skew_Ray_Solver, Human_Triangulation, Human_Triangulation_Condense,
                            Human_Triangulation_Smooth, SecondOrderDynamic, skew_ray_solver_batch, smooth_track)
from .util import Load_Config_Json, Check_If_File_Exist, Load_Video, Draw_Camera_Group, Draw_Skeleton
from .blender import (Human_Triangulation_Blender, Human_Triangulation_Blender_Smooth,
                      Human_Triangulation_To_Blender_Result, save_blender_result)
from .batch import BatchTriangulator
from .pipeline import ShardedTrackPipeline, TrackPipeline
from .tracking import PersonTracker, track_persons_reference
from .fill import fill_joint_track, fill_joint_track_reference
from .despike import despike_joint_track, despike_joint_track_reference
from .refine import refine_joints, refine_joints_reference
from .pose import refine_cameras, refine_cameras_reference, refine_rig
from .reproject import assign_detections, assign_detections_reference
from .seed import pair_cost, pair_cost_reference, seed_persons, seed_persons_reference, seeded_triangulator, triangulate_seeded, triangulate_seeded_reference
from .matched import triangulate_matched, triangulate_matched_reference
from .reproject import match_detections, reproject_reference, reprojection_cost, reprojection_cost_reference, view_residuals   # (reproject.reproject keeps the module's name free)

__all__ = ["Camera", "CameraGroup", "Skew_Ray_Solver", "Human_Triangulation",
           "Human_Triangulation_Condense", "Human_Triangulation_Smooth", "SecondOrderDynamic",
           "skew_ray_solver_batch", "smooth_track", "Load_Config_Json", "Check_If_File_Exist", "Load_Video", "Draw_Camera_Group", "Draw_Skeleton", "BatchTriangulator", "TrackPipeline", "ShardedTrackPipeline", "PersonTracker", "track_persons_reference", "fill_joint_track", "fill_joint_track_reference", "despike_joint_track", "despike_joint_track_reference", "reproject_reference", "reprojection_cost",
           "reprojection_cost_reference", "match_detections", "assign_detections", "assign_detections_reference", "pair_cost", "pair_cost_reference", "seed_persons", "seed_persons_reference", "triangulate_seeded", "triangulate_seeded_reference", "seeded_triangulator", "view_residuals", "refine_joints", "refine_joints_reference", "refine_cameras", "refine_cameras_reference", "refine_rig", "triangulate_matched", "triangulate_matched_reference", "Human_Triangulation_Blender",
           "Human_Triangulation_Blender_Smooth", "Human_Triangulation_To_Blender_Result", "save_blender_result"]
