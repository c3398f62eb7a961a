from bmp.ggnn_jk import ChinGGNN as GGNN       # noqa: F401  (models/chin_ggnn.py)
