"""Encoder registry with the reference's keys (tomosar2height/encoder/__init__.py:3-8); every key is built.
``pointnet_plus_plus`` (encoder/pointnetpp.py) runs for inference, with gradients in ``eval()`` and -- opt-in,
``batch_statistics=True`` -- under ``train()``; ``hourglass`` (encoder/hourglass.py, the image encoder ``model.encoder2:
hourglass`` selects) runs for inference and -- opt-in, ``trainable=True`` / ``stem_gradients=True``, ``norm='group'`` -- with
gradients.  Their forwards raise where training would need what is not built."""
from . import alto, hourglass, pointnet, pointnetpp, unet

encoder_dict = {
    "pointnet_local_pool": pointnet.LocalPoolPointnet,
    "pointnet_plus_plus": pointnetpp.PointNetPlusPlus,
    "hourglass": hourglass.HGFilter,
    "unet": unet.UNet,
}
