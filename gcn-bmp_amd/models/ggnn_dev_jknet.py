from bmp.ggnn_jk import JKNetGGNN as GGNN      # noqa: F401  (models/ggnn_dev_jknet.py)
