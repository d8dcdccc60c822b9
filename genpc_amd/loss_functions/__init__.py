"""The two names the reference's ``loss_functions`` package exports (loss_functions/__init__.py:2-3), and beside
``emdModule`` its form for pairs of different sizes, ``emd_raggedDist`` (not part of the reference's facade)."""
from .Chamfer3D.dist_chamfer_3D import chamfer_3DDist
from .emd.emd_module import emdModule
from .emd.emd_ragged import emd_raggedDist

__all__ = ["chamfer_3DDist", "emdModule", "emd_raggedDist"]
