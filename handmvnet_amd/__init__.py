"""handmvnet_amd -- MI355X-native (gfx950) HandMvNet inference forward pass.

`from handmvnet_amd import HandMvNet` is the drop-in for the reference's
`from models.handmvnet import HandMvNet` on the inference path.
"""
from .spec import HotPathConfig, config_from_params, state_dict_layout  # noqa: F401


def __getattr__(name):
    if name == "HandMvNet":  # lazy: importing the package must not require torch.cuda / the .so
        from .model import HandMvNet
        return HandMvNet
    if name in ("SequenceTracker", "next_crop_boxes", "joints_to_frame", "reproject_crop_boxes"):   # sequences without dataset boxes (tracking.py)
        from . import tracking
        return getattr(tracking, name)
    if name in ("SequenceEvaluator", "labels_to_windows"):   # evaluating a followed sequence (sequence_eval.py)
        from . import sequence_eval
        return getattr(sequence_eval, name)
    if name in ("SubsetSweepEvaluator", "k_of_n", "as_subset_table"):   # camera-subset sweeps (subsets.py)
        from . import subsets
        return getattr(subsets, name)
    if name in ("OcclusionSweepEvaluator", "cell_rects", "grid_variants"):   # occlusion sweeps from raw frames (occlusion.py)
        from . import occlusion
        return getattr(occlusion, name)
    if name in ("ReferenceSweepEvaluator", "each_reference", "rotations", "as_order_table", "pose_consensus"):   # reference-view sweeps (orders.py)
        from . import orders
        return getattr(orders, name)
    if name in ("triangulate", "candidate_table", "batch_triangulate_dlt_torch", "batch_triangulate_dlt_ransac_torch", "triangulate_dlt"):   # absolute position (triangulation.py)
        from . import triangulation
        return getattr(triangulation, name)
    if name in ("heatmap_peaks", "heatmaps_to_coordinates", "confidence_mask"):   # heat-map confidences (confidence.py)
        from . import confidence
        return getattr(confidence, name)
    if name in ("JointsToVertices", "hand_ik", "rigid_unapply"):   # hand pose parameters and MANO vertices (ik.py)
        from . import ik
        return getattr(ik, name)
    if name in ("ManoParams", "ManoSkin"):   # MANO skinning on the device (mano.py)
        from . import mano
        return getattr(mano, name)
    raise AttributeError(name)
