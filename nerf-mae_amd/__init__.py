"""nerf_mae_amd -- MI355X-native (gfx950) engine for the NeRF-MAE 3-D Swin MAE pre-training hot path.

Public surface mirrors the reference (nerf_mae/model/mae/swin_mae3d.py, run_swin_mae3d.py):
`SwinTransformer_MAE3D` / `SwinTransformer_MAE3D_New`, same constructor kwargs, `forward(list_of_grids, is_eval)`
contract and `state_dict()` keys.  All arithmetic runs in libnerfmae_hip.so (hand-written HIP); there is no CPU
fallback and importing the model without the built library fails loudly."""
__version__ = "0.1.0"

_DET_EVAL = ("det_eval_dense", "DetectionEvaluator", "evaluate_box_proposals_recall", "evaluate_box_proposals_ap")
_SEM_EVAL = ("SemanticEvaluator", "sem_eval_dense", "intersection_and_union", "label_class_counts", "class_weights_from_counts", "calculate_class_weights")
_PROJ2D = ("proj2d_cameras", "proj2d_points", "proj2d_terms")
_TWO_STAGE = ("TwoStageDetector", "roi_postprocess_dense", "filter_proposals")


def __getattr__(name):
    # detection evaluation (det_eval.py), loaded on first use so that importing the package stays as light as before
    if name in _DET_EVAL:
        from . import det_eval
        return getattr(det_eval, name)
    if name in _SEM_EVAL:      # voxel-semantics evaluation (sem_eval.py), likewise
        from . import sem_eval
        return getattr(sem_eval, name)
    if name in _TWO_STAGE:     # two-stage detector inference (detector.py), likewise
        from . import detector
        return getattr(detector, name)
    if name in _PROJ2D:        # the 2-D projection term on rows of boxes (proj2d.py), likewise
        from . import proj2d
        return getattr(proj2d, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
