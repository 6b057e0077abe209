"""`finetune.common_dataloader` of the reference (finetune/common_dataloader.py) under its own import name: the TensorFlow-free finetuning
reader of merlot_reserve_amd/finetune_records.py.  The two builders and the two preprocessors keep the reference's roles; jax.process_index() /
local_device_count() are replaced by rank / world (one process per GPU, so a batch has no num_devices axis) and the random draws come from a numpy
Generator."""
from merlot_reserve_amd.finetune_records import finetune_input_fn_builder, finetune_val_input_fn_builder   # noqa: F401
from merlot_reserve_amd.finetune_records import preprocess_tvqa, preprocess_vcr   # noqa: F401

__all__ = ['finetune_input_fn_builder', 'finetune_val_input_fn_builder', 'preprocess_tvqa', 'preprocess_vcr']
