"""`pretrain/validate.py` of the reference under its own import name: merlot_reserve_amd.validate (`python -m merlot_reserve_amd.validate`)."""
from merlot_reserve_amd.validate import main                                                    # noqa: F401
