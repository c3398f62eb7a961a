from bmp.ggnn_dev import DevGGNN as GGNN  # noqa: F401
