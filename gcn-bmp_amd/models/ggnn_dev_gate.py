from bmp.ggnn_gate import GateGGNN as GGNN      # noqa: F401  (models/ggnn_dev_gate.py)
