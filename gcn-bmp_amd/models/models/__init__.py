from bmp.relgcn import GGNNModular as GGNN  # noqa: F401  (models/models/__init__.py:12 of the reference)
from bmp.nfp import NFP                     # noqa: F401  (:13; train_binary.py:41 imports it from here)
