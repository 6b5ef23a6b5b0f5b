"""PER / CER+WER evaluation loops -- mirror of examples/timit/metrics/ctc.py:20-227 (do_eval_per,
do_eval_cer) for the eager model: `session`, `decode_op`, `per_op` are accepted for call compatibility and
ignored; decoding is model.decoder(logits, seq_len, beam_width)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tensorflow_end2end_speech_recognition_amd.utils.io.labels.phone import Idx2phone                 # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.character import Idx2char              # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import sparsetensor2list  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.evaluation.edit_distance import (                # noqa: E402
    compute_per, compute_cer, compute_wer)
from examples.timit.metrics.mapping import Map2phone39                                                # noqa: E402


import numpy as np


def _decode(model, inputs, seq_len, beam_width, task=None, lm_kw=None):
    """task: None (single-task model) | 'main' | 'sub' (MultitaskCTC: which head's decode to return).  lm_kw: the
    lm / lm_weight / insertion_bonus keywords of CTC.decoder (an extension; None or empty: today's decode)."""
    lm_kw = lm_kw or {}
    B = inputs.shape[0]
    dummy = np.zeros((B, 1), dtype=np.int64)                    # labels are not needed for the logits
    if task is None:
        _, logits = model.compute_loss(inputs, dummy, seq_len, keep_prob=1.0, is_training=False)
        # the logits of a model that subsamples in time have output_seq_len(seq_len) frames; a model object without the
        # method (these loops take any object with compute_loss / decoder) does not subsample: seq_len
        out_len = model.output_seq_len(seq_len) if hasattr(model, 'output_seq_len') else seq_len
        dec = model.decoder(logits, out_len, beam_width=beam_width, **lm_kw)
    else:
        _, logits_main, logits_sub = model.compute_loss(inputs, dummy, dummy, seq_len, keep_prob=1.0,
                                                        is_training=False)
        dec = model.decoder(logits_main, logits_sub, seq_len, beam_width=beam_width, **lm_kw)[0 if task == 'main' else 1]
    return [np.asarray(h, dtype=np.int64) for h in sparsetensor2list(dec, B)]


def _lm_kw(lm, lm_weight, insertion_bonus):
    """CTC.decoder's fusion keywords, or {} when none is set (the call is then exactly the one without them)."""
    if lm is None and not lm_weight and not insertion_bonus:
        return {}
    return dict(lm=lm, lm_weight=lm_weight, insertion_bonus=insertion_bonus)


def do_eval_per(session, decode_op, per_op, model, dataset, label_type, is_test=False, eval_batch_size=None,
                progressbar=False, is_multitask=False, map_dir=None, beam_width=1, lm=None, lm_weight=0.0,
                insertion_bonus=0.0):
    """Mean phone error rate on the 39-phone set (:20-124).  map_dir: directory with <label_type>.txt and
    phone2phone.txt (the reference hard-codes '../metrics/mapping_files/')."""
    map_dir = map_dir or '../metrics/mapping_files'
    lm_kw = _lm_kw(lm, lm_weight, insertion_bonus)
    batch_size_original = dataset.batch_size
    dataset.reset()
    if eval_batch_size is not None:
        dataset.batch_size = eval_batch_size
    eval_label_type = dataset.label_type_sub if is_multitask else getattr(dataset, 'label_type', label_type)
    idx2phone_train = Idx2phone(os.path.join(map_dir, label_type + '.txt'))
    idx2phone_eval = Idx2phone(os.path.join(map_dir, eval_label_type + '.txt'))
    p2p = os.path.join(map_dir, 'phone2phone.txt')
    p2p = p2p if os.path.isfile(p2p) else None
    to39_train, to39_eval = Map2phone39(label_type, p2p), Map2phone39(eval_label_type, p2p)
    per_sum = 0.0
    for data, is_new_epoch in dataset:
        if is_multitask:
            inputs, _, labels_true, inputs_seq_len, _ = data
        else:
            inputs, labels_true, inputs_seq_len, _ = data
        hyps = _decode(model, inputs[0], inputs_seq_len[0], beam_width, 'sub' if is_multitask else None, lm_kw)
        for b in range(inputs[0].shape[0]):
            pred = to39_train(idx2phone_train(hyps[b]).split(' ')) if len(hyps[b]) else []
            if is_test:
                true = labels_true[0][b][0].split(' ')
            else:
                true = idx2phone_eval(labels_true[0][b]).split(' ')
            true = to39_eval(true)
            # NB the reference passes the hypothesis as `ref` (:106-108), i.e. normalises by ITS length; an empty
            # hypothesis (ZeroDivisionError there) scores 1.0 here
            per_sum += compute_per(ref=pred, hyp=true, normalize=True) if len(pred) else float(len(true) > 0)
        if is_new_epoch:
            break
    if eval_batch_size is not None:
        dataset.batch_size = batch_size_original
    return per_sum / len(dataset)


def do_eval_cer(session, decode_op, model, dataset, label_type, is_test=False, eval_batch_size=None,
                progressbar=False, is_multitask=False, map_dir=None, beam_width=1, lm=None, lm_weight=0.0,
                insertion_bonus=0.0):
    """(mean CER, mean WER) (:127-227): '_' separates words; punctuation is stripped before scoring."""
    map_dir = map_dir or '../metrics/mapping_files'
    lm_kw = _lm_kw(lm, lm_weight, insertion_bonus)
    batch_size_original = dataset.batch_size
    dataset.reset()
    if eval_batch_size is not None:
        dataset.batch_size = eval_batch_size
    if label_type == 'character':
        idx2char = Idx2char(os.path.join(map_dir, 'character.txt'))
    elif label_type == 'character_capital_divide':
        idx2char = Idx2char(os.path.join(map_dir, 'character_capital_divide.txt'), capital_divide=True, space_mark='_')
    else:
        raise ValueError('label_type must be character or character_capital_divide')
    cer_sum = wer_sum = 0.0
    for data, is_new_epoch in dataset:
        if is_multitask:
            inputs, labels_true, _, inputs_seq_len, _ = data
        else:
            inputs, labels_true, inputs_seq_len, _ = data
        hyps = _decode(model, inputs[0], inputs_seq_len[0], beam_width, 'main' if is_multitask else None, lm_kw)
        for b in range(inputs[0].shape[0]):
            if is_test:
                str_true = labels_true[0][b][0]
            else:
                str_true = idx2char(labels_true[0][b], padded_value=dataset.padded_value)
            str_pred = re.sub(r'[_]+', '_', idx2char(hyps[b]))
            str_true = re.sub(r'[\'\":;!?,.-]+', '', str_true)
            str_pred = re.sub(r'[\'\":;!?,.-]+', '', str_pred)
            wer_sum += compute_wer(hyp=str_pred.split('_'), ref=str_true.split('_'), normalize=True)
            cer_sum += compute_cer(str_pred=re.sub(r'[_]+', '', str_pred), str_true=re.sub(r'[_]+', '', str_true),
                                   normalize=True)
        if is_new_epoch:
            break
    if eval_batch_size is not None:
        dataset.batch_size = batch_size_original
    return cer_sum / len(dataset), wer_sum / len(dataset)
