"""`pretrain/train.py` of the reference under its own import name: the loop lives in merlot_reserve_amd.train (`python -m merlot_reserve_amd.train`)."""
from merlot_reserve_amd.train import main                                                       # noqa: F401
