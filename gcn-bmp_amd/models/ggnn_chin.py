from bmp.relgcn import GGNNModular as GGNN     # noqa: F401  (models/ggnn_chin.py)
