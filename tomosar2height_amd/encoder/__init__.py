"""Encoder registry with the reference's keys (tomosar2height/encoder/__init__.py:3-8); every key is built.
``pointnet_plus_plus`` (encoder/pointnetpp.py) and ``hourglass`` (encoder/hourglass.py, the image encoder ``model.encoder2:
hourglass`` selects) run for inference only: their forwards raise where training would need a backward that is not built
(DESIGN.md section 8)."""
from . import alto, hourglass, pointnet, pointnetpp, unet

encoder_dict = {
    "pointnet_local_pool": pointnet.LocalPoolPointnet,
    "pointnet_plus_plus": pointnetpp.PointNetPlusPlus,
    "hourglass": hourglass.HGFilter,
    "unet": unet.UNet,
}
