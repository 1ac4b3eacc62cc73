"""Encoder registry with the reference's keys (tomosar2height/encoder/__init__.py:3-8).  ``pointnet_plus_plus`` is built for
inference (encoder/pointnetpp.py; ``forward`` under ``train()`` raises).  ``hourglass``, which no reference config selects, is
out of the hot-path scope and raises a clear error instead of silently missing."""
from . import alto, pointnet, pointnetpp, unet


class _NotBuilt:
    def __init__(self, name):
        self.name = name

    def __call__(self, *args, **kwargs):
        raise NotImplementedError(f"encoder '{self.name}' is outside the MI355X hot-path scope (SURVEY.md section 8)")


encoder_dict = {
    "pointnet_local_pool": pointnet.LocalPoolPointnet,
    "pointnet_plus_plus": pointnetpp.PointNetPlusPlus,
    "hourglass": _NotBuilt("hourglass"),
    "unet": unet.UNet,
}
