from bmp.ggnn_jk import JKGruGGNN as GGNN      # noqa: F401  (models/ggnn_dev_jk_gru.py)
