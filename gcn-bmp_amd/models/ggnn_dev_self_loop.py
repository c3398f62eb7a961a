from bmp.ggnn_dev import SelfLoopGGNN as GGNN  # noqa: F401
