"""Which test covers which export: every function include/mreserve_hip.h declares names the test file(s) that call it directly (no GPU).

LEDGER maps an export to (the Python names tests reach it by, the test files).  The key set must equal the header's; every file must exist and must
contain the export's C name or one of its wrapper names; every wrapper must be defined in the binding module that calls the export.  An export added
later without a named test fails here."""
import os
import re

from test_cabi_exports import ROOT, declared_symbols

K, F32K, G3, EX, DIRECT = 'test_kernels_gpu.py', 'test_f32_kernels_gpu.py', 'test_gemm3_gpu.py', 'test_gemm_exact_gpu.py', 'test_exports_direct_gpu.py'
CABI, DIST, REC, RING = 'test_cabi_exports.py', 'test_dist_gpu.py', 'test_records.py', 'test_metrics_ring_gpu.py'
ROWS = 'test_rowops_exact_gpu.py'           # element-exact: LayerNorm, reductions, row kernels

LEDGER = {
    # library, handles, options
    'mr_version': ((), (CABI,)),
    'mr_last_error': ((), (CABI,)),
    'mr_create': (('Handle',), (CABI,)),
    'mr_destroy': (('Handle',), (CABI,)),
    'mr_make_current': (('Handle',), (CABI,)),
    'mr_get_current': (('Handle',), (CABI,)),
    'mr_handle_set_option': (('Handle',), (CABI,)),
    'mr_handle_get_option': (('Handle',), (CABI,)),
    'mr_set_option': (('set_option',), (CABI, EX)),
    'mr_get_option': (('get_option',), (CABI, EX)),
    'mr_last_gemm_kernel': ((), (EX, G3)),
    # GEMM
    'mr_gemm': (('gemm',), (EX, G3, K)),
    'mr_gemm_grouped': (('gemm_grouped',), (EX, G3, K)),
    'mr_gemm_colsum_rows': (('gemm_colsum_job',), (EX, G3, K)),
    'mr_gemm_colsum_supported': (('gemm_colsum_job',), (K,)),
    # LayerNorm, reductions
    'mr_layernorm_fwd': (('layernorm_fwd',), (K, ROWS)),
    'mr_layernorm_bwd': (('layernorm_bwd',), (K, ROWS)),
    'mr_layernorm_bwd_workspace': (('layernorm_bwd_workspace',), (K, ROWS)),
    'mr_layernorm_bwd_nparts': (('layernorm_bwd',), (K, ROWS)),
    'mr_colsum': (('colsum',), (K, ROWS)),
    'mr_colsum_workspace': (('colsum_workspace',), (K, ROWS)),
    'mr_colsum_nparts': (('colsum',), (K, ROWS)),
    'mr_reduce_partials': (('reduce_partials',), (K, ROWS)),
    # attention
    'mr_attention_fwd': (('attention_fwd',), (K,)),
    'mr_attention_bwd': (('attention_bwd',), (K,)),
    'mr_attention_bwd_colsum_rows': (('attention_bwd',), (K,)),
    'mr_attention_fwd_dense_mask': (('attention_fwd_dense_mask',), (K,)),
    'mr_attention_bwd_dense_mask': (('attention_bwd_dense_mask',), (K,)),
    'mr_attention_bwd_dense_mask_workspace': (('attention_bwd_dense_mask',), (K,)),
    'mr_poolattn_fwd': (('poolattn_fwd',), (K, ROWS)),
    'mr_poolattn_bwd': (('poolattn_bwd',), (K, ROWS)),
    # row operations
    'mr_segment_sum': (('segment_sum',), (K, ROWS)),
    'mr_rows_mean_fwd': (('rows_mean_fwd',), (K, ROWS)),
    'mr_rows_mean_bwd': (('rows_mean_bwd',), (K, ROWS)),
    'mr_pad_cols': (('pad_cols',), (K, ROWS)),
    'mr_fill_rows': (('fill_rows',), (K, ROWS)),
    'mr_sum_rows_strided': (('sum_rows_strided',), (K, ROWS)),
    'mr_add_bf16': (('add_',), (K, ROWS)),
    'mr_unit_norm_scale_fwd': (('unit_norm_scale_fwd',), (K, ROWS)),
    'mr_unit_norm_scale_bwd': (('unit_norm_scale_bwd',), (K, ROWS)),
    # losses
    'mr_contrastive_lse': (('contrastive_lse',), (K,)),
    'mr_masked_lm_xent': (('masked_lm_xent',), (DIRECT,)),
    'mr_softmax_xent': (('softmax_xent',), (DIRECT,)),
    'mr_cast_f32_to_bf16': (('cast_f32_to_bf16',), (K,)),
    'mr_split_f32_to_bf16_hilo': (('split_hilo',), (DIRECT,)),
    'mr_split_f32_to_bf16_hilo_rows': (('split_hilo_rows',), (DIRECT,)),
    'mr_metrics_push': (('metrics_push',), (RING,)),
    # optimizer
    'mr_adam_bf16_update': (('adam_bf16_update',), (K, DIRECT)),
    'mr_adam_bf16_update_finetune': (('adam_bf16_update_finetune',), (DIRECT,)),
    'mr_adam_bf16_update_dev': (('adam_bf16_update_dev',), (DIRECT,)),
    'mr_adam_f32grad_update_dev': ((), (DIRECT,)),
    'mr_nan_to_num_bf16': (('nan_to_num_',), (DIRECT,)),
    'mr_cast_f32_to_bf16_params': (('cast_params',), (DIRECT,)),
    'mr_transpose_leaves': (('transpose_leaves',), (DIRECT,)),
    # fp32 path
    'mr_f32_gemm': (('gemm',), (F32K,)),
    'mr_f32_layernorm_fwd': (('layernorm_fwd',), (F32K,)),
    'mr_f32_layernorm_bwd': (('layernorm_bwd',), (F32K,)),
    'mr_f32_colsum': (('colsum',), (F32K,)),
    'mr_f32_attention_fwd': (('attention_fwd',), (F32K,)),
    'mr_f32_attention_bwd': (('attention_bwd',), (F32K,)),
    'mr_f32_poolattn_fwd': (('poolattn_fwd',), (F32K,)),
    'mr_f32_poolattn_bwd': (('poolattn_bwd',), (F32K,)),
    'mr_f32_segment_sum': (('segment_sum',), (F32K,)),
    'mr_f32_rows_mean_fwd': (('rows_mean_fwd',), (F32K,)),
    'mr_f32_rows_mean_bwd': (('rows_mean_bwd',), (F32K,)),
    'mr_f32_unit_norm_scale_fwd': (('unit_norm_scale_fwd',), (F32K,)),
    'mr_f32_unit_norm_scale_bwd': (('unit_norm_scale_bwd',), (F32K,)),
    'mr_f32_fill_rows': (('fill_rows',), (F32K,)),
    'mr_f32_sum_rows_strided': (('sum_rows_strided',), (F32K,)),
    'mr_f32_axpby': ((), (DIRECT,)),
    'mr_f32_nan_to_num': ((), (DIRECT,)),
    # collectives (dist.NativeComm: its constructor makes the id, initialises, and checks rank and world; close() destroys)
    'mr_comm_unique_id': (('NativeComm',), (DIST,)),
    'mr_comm_init': (('NativeComm',), (DIST,)),
    'mr_comm_destroy': (('NativeComm',), (DIST,)),
    'mr_comm_rank': (('NativeComm',), (DIST,)),
    'mr_comm_world': (('NativeComm',), (DIST,)),
    'mr_allreduce_mean_bf16': (('allreduce_mean',), (DIST,)),
    'mr_allreduce_mean_f32': (('allreduce_mean_f32',), (DIST,)),
    'mr_allgather': (('gather_embeddings',), (DIST,)),
    'mr_reducescatter_sum': (('scatter_grad',), (DIST,)),
    'mr_reducescatter_sum_f32': (('scatter_grad',), (DIST,)),
    # host-side record I/O
    'mr_crc32c': ((), (REC,)),
    'mr_crc32c_masked': ((), (REC,)),
    'mr_tfrecord_scan': (('read_tfrecord',), (REC,)),
}

BINDINGS = ('ops.py', 'dist.py', 'records.py')


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_export_names_its_test():
    assert set(LEDGER) == set(declared_symbols()), sorted(set(LEDGER) ^ set(declared_symbols()))


def test_named_tests_exist_and_call_the_export():
    bindings = {b: _read('merlot_reserve_amd', b) for b in BINDINGS}
    for export, (wrappers, files) in LEDGER.items():
        assert files, export
        for w in wrappers:          # a wrapper is a def / class / method of the binding module that calls the export
            assert any(re.search(rf'^\s*(def|class) {re.escape(w)}\b', src, flags=re.M) and re.search(rf'\b{export}\b', src)
                       for src in bindings.values()), f'{export}: no binding defines {w} and calls the export'
        for fname in files:
            path = os.path.join(ROOT, 'tests', fname)
            assert os.path.isfile(path), f'{export}: {fname} does not exist'
            text = _read('tests', fname)
            names = (export,) + tuple(wrappers)
            assert any(re.search(rf'\b{re.escape(n)}\b', text) for n in names), f'{export}: {fname} mentions none of {names}'


def test_a_new_export_without_a_test_is_caught():
    header = set(declared_symbols()) | {'mr_some_new_export'}
    assert set(LEDGER) != header
