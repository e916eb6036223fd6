"""tcdiff_amd: MI355X-native (gfx950) implementation of TCDiff's denoising hot path.

    from tcdiff_amd import DanceDecoder, GaussianDiffusion     # drop-ins for model.model / model.diffusion
    from tcdiff_amd import AIOZDataset                         # drop-in for dataset.group_dataset
"""
from .model import DanceDecoder  # noqa: F401
from .diffusion import GaussianDiffusion, EMA  # noqa: F401
from .adan import Adan  # noqa: F401
from .fk import SMPLSkeleton, ax_from_6v  # noqa: F401
from .navigator import TrajDecoder, TrajTrainer, TrajAdamW, traj_loss  # noqa: F401
from .dataset import AIOZDataset, process_motion  # noqa: F401
from .metrics import motion_metrics, beats_from_cond, evaluate_samples, summarize  # noqa: F401
from .draw import camera, draw_dance, draw_samples, write_apng  # noqa: F401
from .set_metrics import SetStats, kinetic_features, fit_reference, set_scores, evaluate_set, reference_from_joints  # noqa: F401
from .set_metrics import GEOMETRIC_TABLE, geometric_features, geometric_table, evaluate_set_all  # noqa: F401
from .music import music_features, assemble_cond, beat_track, music_cond, chroma_cqt, estimate_tuning, wav_cond  # noqa: F401
from .gltf import animation_block, build_glb, write_glb, write_glb_out, convert_fk_out  # noqa: F401
from .body import BodyModel, load_body_model, skin  # noqa: F401
from .shade import vertex_normals, draw_bodies, draw_body_samples  # noqa: F401
from .video import JpegFrames, encode_jpeg, jpeg_tables, pcm16, write_avi, clip_audio  # noqa: F401
from .footlock import FootLock, foot_lock  # noqa: F401
from .group_metrics import group_metrics, pairs, capsule_radii, radii_from_body, evaluate_group  # noqa: F401
from .apart import Apart, keep_apart  # noqa: F401
from .ground import Ground, ground, ground_metrics  # noqa: F401
from .mesh_contact import mesh_contact, evaluate_mesh_contact  # noqa: F401
from .self_contact import self_contact, self_pairs, pair_index, pair_of, pair_mask, evaluate_self_contact  # noqa: F401
from .smooth import Smooth, smooth, smoothness, evaluate_smoothness, savgol_table  # noqa: F401
from .choreo import Plan, plan, trajectory_error, formation  # noqa: F401
from .beat_sync import BeatSync, beat_sync, motion_beats, gaussian_table  # noqa: F401
from .audio import WavData, read_wav, decode, resample, slice_audio, load_audio  # noqa: F401

__all__ = ["DanceDecoder", "GaussianDiffusion", "EMA", "Adan", "SMPLSkeleton", "ax_from_6v", "TrajDecoder", "TrajTrainer", "TrajAdamW",
           "traj_loss", "AIOZDataset", "process_motion", "motion_metrics", "beats_from_cond", "evaluate_samples", "summarize",
           "camera", "draw_dance", "draw_samples", "write_apng", "SetStats", "kinetic_features", "fit_reference", "set_scores",
           "evaluate_set", "reference_from_joints", "GEOMETRIC_TABLE", "geometric_features", "geometric_table", "evaluate_set_all",
           "music_features", "assemble_cond",
           "beat_track", "music_cond", "chroma_cqt", "estimate_tuning", "wav_cond", "WavData", "read_wav", "decode", "resample",
           "slice_audio", "load_audio", "animation_block", "build_glb", "write_glb", "write_glb_out", "convert_fk_out",
           "BodyModel", "load_body_model", "skin", "vertex_normals", "draw_bodies", "draw_body_samples",
           "group_metrics", "pairs", "capsule_radii", "radii_from_body", "evaluate_group", "Apart", "keep_apart",
           "Ground", "ground", "ground_metrics", "mesh_contact", "evaluate_mesh_contact",
           "self_contact", "self_pairs", "pair_index", "pair_of", "pair_mask", "evaluate_self_contact",
           "Smooth", "smooth", "smoothness", "evaluate_smoothness", "savgol_table",
           "Plan", "plan", "trajectory_error", "formation",
           "BeatSync", "beat_sync", "motion_beats", "gaussian_table"]
