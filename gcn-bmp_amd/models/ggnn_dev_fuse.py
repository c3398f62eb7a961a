from bmp.ggnn_gate import FuseGGNN as GGNN      # noqa: F401  (models/ggnn_dev_fuse.py)
