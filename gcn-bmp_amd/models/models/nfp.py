from bmp.nfp import NFP, NFPReadout, NFPUpdate  # noqa: F401  (models/models/nfp.py)
