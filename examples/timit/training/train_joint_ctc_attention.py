#!/usr/bin/env python
"""Train the joint CTC-attention model on TIMIT -- the recipe of
examples/timit/training/train_joint_ctc_attention.py.

    python examples/timit/training/train_joint_ctc_attention.py <config.yml> <model_save_path>

As train_attention.py with the joint dataset (attention targets + CTC targets of the same utterances) and the
`lambda_weight` interpolation of the two losses; evaluation uses the attention decoder (is_jointctcatt=True)."""
import sys
from os.path import abspath, dirname, isfile, join

import numpy as np
import yaml

ROOT = dirname(dirname(dirname(dirname(abspath(__file__)))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from examples.timit.data.load_dataset_joint_ctc_attention import Dataset                                     # noqa: E402
from examples.timit.metrics.attention import do_eval_per, do_eval_cer                                        # noqa: E402
from examples.timit.metrics.mapping_files import write_mapping_files                                         # noqa: E402
from examples.timit.training._common import NUM_CLASSES, new_run_directory, run_with_log, training_loop       # noqa: E402
from examples.timit.training.train_attention import (attention_ler, make_datasets, model_kwargs, run_name,    # noqa: E402
                                                     scheduled_sampling_prob)
from tensorflow_end2end_speech_recognition_amd.models.attention.joint_ctc_attention import JointCTCAttention  # noqa: E402
from tensorflow_end2end_speech_recognition_amd.utils.io.labels.sparsetensor import list2sparsetensor         # noqa: E402


def do_train(model, params):
    map_dir = params.get('map_dir') or join(model.save_path, 'mapping_files')
    if not isfile(join(map_dir, 'phone2phone.txt')):
        write_mapping_files(map_dir)
    train_data, dev_data, test_data = make_datasets(Dataset, params, map_dir)
    is_char = 'char' in params['label_type']
    kp = [1 - float(params[k]) for k in ('dropout_encoder', 'dropout_decoder', 'dropout_embedding')]

    steps = [0]

    def losses(data, keep, is_training, ss=0.0):
        inputs, att_labels, ctc_labels, inputs_seq_len, att_labels_seq_len, _ = data
        ctc_st = list2sparsetensor(ctc_labels[0], padded_value=-1)
        return model.compute_loss(inputs[0], att_labels[0], ctc_st, inputs_seq_len[0], att_labels_seq_len[0],
                                  keep[0], keep[1], keep[2], is_training=is_training,
                                  **(dict(scheduled_sampling_prob=ss) if ss else {}))

    def train_step(data, learning_rate):
        ss = scheduled_sampling_prob(params, steps[0])
        steps[0] += 1
        loss = losses(data, kp, True, ss)[0]
        model.train(loss, optimizer=params['optimizer'], learning_rate=learning_rate)

    def monitor(data):
        loss, _, _, out_train, out_infer = losses(data, (1.0, 1.0, 1.0), False)
        _, ids_infer = model.decode(out_train, out_infer)
        ids_infer = np.asarray(ids_infer.cpu() if hasattr(ids_infer, 'cpu') else ids_infer)
        return float(loss), attention_ler(model, data[1][0], data[4][0], ids_infer)

    def evaluate(is_test):
        ev = dict(session=None, decode_op=None, model=model, dataset=test_data if is_test else dev_data,
                  label_type=params['label_type'], is_test=is_test, eval_batch_size=1, map_dir=map_dir,
                  is_jointctcatt=True)
        if is_char:
            cer, wer = do_eval_cer(**ev)
            print('  WER: %f %%' % (wer * 100))
            return cer
        return do_eval_per(per_op=None, **ev)

    return training_loop(model, params, train_data, dev_data, train_step, monitor, evaluate,
                         'CER' if is_char else 'PER')


def joint_run_name(params):
    name = run_name(params) + '_lambda' + str(params['lambda_weight'])
    if params.get('ctc_label_smoothing_prob'):
        name += '_ctcls' + str(params['ctc_label_smoothing_prob'])
    return name


def main(config_path, model_save_path, log_to_file=True):
    with open(config_path, 'r') as f:
        params = yaml.safe_load(f)['param']
    if params['label_type'] not in NUM_CLASSES:
        raise TypeError
    params['num_classes'] = NUM_CLASSES[params['label_type']]
    model = JointCTCAttention(lambda_weight=params['lambda_weight'],
                              ctc_label_smoothing_prob=float(params.get('ctc_label_smoothing_prob') or 0.0),
                              **model_kwargs(params))
    model.name = joint_run_name(params)
    model.save_path = new_run_directory(join(model_save_path, 'joint_ctc_attention', params['label_type'], model.name),
                                        config_path)
    result = run_with_log(lambda: do_train(model, params), model.save_path, log_to_file)
    result.update(save_path=model.save_path, model=model)
    return result


if __name__ == '__main__':
    args = sys.argv
    if len(args) != 3:
        raise ValueError('Length of args should be 3.')
    main(config_path=args[1], model_save_path=args[2])
