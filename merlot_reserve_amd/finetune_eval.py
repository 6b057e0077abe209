"""Validation epoch and prediction files of the two finetuning tasks: val_epoch of finetune/vcr/qa_qar_joint_finetune.py:208-239 (V) and
finetune/tvqa/tvqa_finetune.py:316-361 (T), and the files of the two submit_to_leaderboard.py scripts (VS = finetune/vcr/..., TS = finetune/tvqa/...).

    val_epoch(model_or_state, val_iter, task) -> (accuracies, rows)     one row per example: {'id', 'preds', 'logprobs', 'labels'}
    write_predictions(rows, path)                                        JSON lines of those rows
    write_vcr_submission(rows, path)                                     the CSV of VS:129-146
    write_tvqa_submission({'val': rows, 'test': rows}, directory, ...)   the JSON files of TS:205-234

The device work is the forward-only program of the model (finetune.pred_step / tvqa.pred_step); everything here is host arithmetic on B x 2 x A
(VCR) or 2 x B x A (TVQA) numbers.  No pandas: the reference's frames are a mean of equalities and one sort."""
import json
import math
import os

import numpy as np

TASKS = ('vcr', 'tvqa')
ACCURACY_KEYS = {'vcr': ('qa_acc', 'qar_acc'), 'tvqa': ('text_acc', 'audio_acc', 'joint_acc')}


def rows_of(ids, pred, labels, task):
    """The prediction rows of one batch from pred_step's output; examples whose id is 'pad' are skipped (V:227, T:344)."""
    rows = []
    labels = np.asarray(labels)
    for i, id_i in enumerate(ids):
        if id_i == 'pad':
            continue
        if task == 'vcr':
            rows.append({'id': id_i, 'preds': [int(p) for p in pred['preds'][i]], 'logprobs': [[float(x) for x in r] for r in pred['logprobs'][i]],
                         'labels': [int(x) for x in labels[i]]})
        else:
            rows.append({'id': id_i, 'preds': {k: int(pred[f'preds_{k}'][i]) for k in ('text', 'audio', 'joint')},
                         'logprobs': {k: [float(x) for x in pred[f'logprobs_{k}'][i]] for k in ('text', 'audio')}, 'labels': int(labels[i])})
    return rows


def accuracies(rows, task):
    """V:232-239: qa_acc / qar_acc; T:350-361: text_acc / audio_acc / joint_acc -- the mean of pred == label over the rows."""
    n = len(rows)
    if task == 'vcr':
        hits = {'qa_acc': sum(r['preds'][0] == r['labels'][0] for r in rows), 'qar_acc': sum(r['preds'][1] == r['labels'][1] for r in rows)}
    else:
        hits = {f'{k}_acc': sum(r['preds'][k] == r['labels'] for r in rows) for k in ('text', 'audio', 'joint')}
    return {k: (v / n if n else math.nan) for k, v in hits.items()}


def _pred_fn(model_or_state, task):
    from . import finetune, tvqa
    model = finetune._model_of(model_or_state)
    step = finetune.pred_step if task == 'vcr' else tvqa.pred_step
    keys = model.engine_cls.device_keys

    def fn(batch):
        batch = dict(batch)
        for k in keys:                                         # the float arrays of a reader's batch are host tensors
            batch[k] = batch[k].to(model.device, non_blocking=True)
        return step(model, batch)
    return fn


def val_epoch(model_or_state, val_iter, task, pred_fn=None):
    """One pass over val_iter (finetune_records.finetune_val_input_fn_builder: (ids, batch) with the last batch padded by 'pad' ids).
    Returns (the task's accuracies, the prediction rows in the order read)."""
    assert task in TASKS, task
    pred_fn = pred_fn or _pred_fn(model_or_state, task)
    rows = []
    for ids, batch in val_iter:
        rows += rows_of(ids, pred_fn(batch), batch['labels'], task)
    return accuracies(rows, task), rows


def write_predictions(rows, path):
    with open(path, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
    return path


def read_predictions(path):
    return [json.loads(line) for line in open(path)]


def write_vcr_submission(rows, path):
    """VS:129-146.  annot_id = the first two '-' fields of the id, the conditionee = the text after the last '_'; one line per annot_id with the
    probabilities (exp of the fp32 log-probabilities) in the columns answer_i and rationale_conditioned_on_{c}_{i}, the lines sorted by the
    integer in the annot_id.  Every line must fill every column (the reference asserts no nulls)."""
    out, columns = {}, []
    for r in rows:
        probs = np.exp(np.asarray(r['logprobs'], dtype=np.float32))
        A = probs.shape[-1]
        annot_id, cond = '-'.join(r['id'].split('-')[:2]), r['id'].split('_')[-1]
        sub = {f'answer_{i}': probs[0, i] for i in range(A)}
        sub.update({f'rationale_conditioned_on_{cond}_{i}': probs[1, i] for i in range(A)})
        for k in sub:
            if k not in columns:
                columns.append(k)
        out.setdefault(annot_id, {}).update(sub)
    order = sorted(out, key=lambda a: int(a.split('-')[1]))
    with open(path, 'w') as f:
        f.write(','.join(['annot_id'] + columns) + '\n')
        for a in order:
            missing = [c for c in columns if c not in out[a]]
            assert not missing, f'{a}: no value for {missing}'
            f.write(','.join([a] + [repr(float(out[a][c])) for c in columns]) + '\n')
    return path


def write_tvqa_submission(rows_by_split, directory, model_size='Base'):
    """TS:205-234: for each of text / audio / joint a folder with prediction_val.json and prediction_test_public.json ({question id: predicted
    answer}, the id cut at '~') and meta.json, and the folder's files zipped beside it.  rows_by_split: {'val': rows, 'test': rows}; a split
    that is not given gets no file (and none in the archive) rather than an empty one."""
    import zipfile
    unknown = set(rows_by_split) - {'val', 'test'}
    assert not unknown, f'unknown split {sorted(unknown)}: val or test'
    suffixes = {'text': '(subtitles)', 'audio': '(audio)', 'joint': '(subtitles and audio)'}
    names = {'val': 'prediction_val.json', 'test': 'prediction_test_public.json'}
    written = []
    for sub in ('text', 'audio', 'joint'):
        folder = os.path.join(str(directory), sub)
        os.makedirs(folder, exist_ok=True)
        files = {names[split]: {r['id'].split('~')[0]: r['preds'][sub] for r in rows_by_split[split]} for split in ('val', 'test') if split in rows_by_split}
        files['meta.json'] = {'model_name': f'MerlotReserve-{model_size} {suffixes[sub]}', 'is_ensemble': False, 'with_ts': True,
                              'show_on_leaderboard': True, 'author': 'Anonymous', 'institution': 'Anonymous',
                              'description': 'A {}-sized model, given {} at test time'.format(model_size, suffixes[sub].strip('()')),
                              'paper_link': '', 'code_link': ''}
        for name, obj in files.items():
            with open(os.path.join(folder, name), 'w') as f:
                json.dump(obj, f)
        with zipfile.ZipFile(os.path.join(str(directory), f'{sub}.zip'), 'w') as z:
            for name in files:
                z.write(os.path.join(folder, name), name)
        written.append(folder)
    return written
