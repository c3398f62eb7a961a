from bmp.gin import GIN, GINUpdate      # noqa: F401  (models/gin.py)
from bmp.relgcn import GGNNReadout     # noqa: F401  (models/gin.py:9-55 carries its own copy of the readout)
