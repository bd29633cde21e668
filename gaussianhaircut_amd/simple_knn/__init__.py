"""Drop-in for the reference's ``simple_knn`` package (imported at ``src/scene/gaussian_model.py:21`` as
``from simple_knn._C import distCUDA2``), backed by ``libghr_hip.so``: see ``_C.distCUDA2``."""
from ._C import distCUDA2  # noqa: F401
