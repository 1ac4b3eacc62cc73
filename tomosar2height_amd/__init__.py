"""tomosar2height_amd -- MI355X (gfx950) implementation of the dual-topology point-cloud hot path of
zhu-xlab/tomosar2height behind the reference's own module interface.

    from tomosar2height_amd import TomoSAR2Height, encoder_dict, decoder_dict

The device arithmetic lives in ``libt2h_hip.so`` (C ABI: include/t2h.h, sources: csrc/*.hip); there is no CPU
path in this package.
"""
from .model import TomoSAR2Height
from .decoder import decoder_dict
from .encoder import encoder_dict
from .tile import TileIndex
from .evaluator import DSMEvaluator, dilate_mask
from .instances import BuildingEvaluator, label_components, segment_medians
from .cloud_instances import CloudBuildingEvaluator, assign_points, point_medians
from .interpolate import CloudIndex, delaunay_dsm, grid_knn, grid_simplex, idw_dsm, linear_dsm, nearest_dsm
from ._lib import allow_library_fallback, fallback_counts

__all__ = ["TomoSAR2Height", "decoder_dict", "encoder_dict", "TileIndex", "DSMEvaluator", "dilate_mask",
           "BuildingEvaluator", "label_components", "segment_medians", "CloudBuildingEvaluator", "assign_points",
           "point_medians", "CloudIndex", "grid_knn", "nearest_dsm", "idw_dsm",
           "linear_dsm", "delaunay_dsm", "grid_simplex", "allow_library_fallback", "fallback_counts"]
